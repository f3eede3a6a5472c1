// The read-back arena: everything the host reads once per outer iteration, in one piece so that one copy fetches it.
//   [8 objective slots per mode | 2 per tensor | 8 residual slots per mode | 16 scratch | 4 EM statistics per tensor
//    | 4 held-out sums per tensor | 8 ranking-metric sums per tensor]
//   | AdmmCtl[n_modes + n_couplings + 1] | per PARAFAC2 block: res (K + 1), q (4 K), regv (K)
// ArenaLayout holds the offsets (Engine::model_end fills it); ArenaView hands out typed pointers from a base pointer,
// the device arena and its pinned host copy alike.
#pragma once
#include <vector>

#include "common.h"
#include "small.h"

namespace aoadmm {

constexpr int kSlotsPerMode = 8;      // objective slots
constexpr int kSlotsPerTensor = 2;
constexpr int kResidPerMode = 8;      // ADMM residual slots
constexpr int kScratchSlots = 16;     // one-off sums outside the outer loop (||X||^2, the synthetic generator's norms)

// objective slots of a mode (mode_obj)
enum ModeObj {
  kObjFacSq = 0,      // ||fac||^2
  kObjFacZSq = 1,     // ||fac - Z||^2
  kObjCouplGap = 2,   // ||Tf(fac) - Sd(Delta)||^2
  kObjRegValue = 3,   // reg_func(fac)
  kObjImageSq = 4,    // ||Tf(fac)||^2 where the image is not the factor itself
};
// objective slots of a tensor (tensor_obj): the last_mttkrp / last_had form of the residual
enum TensorObj {
  kObjMttkrpDot = 0,  // <A, fac> = w * f_2
  kObjHadDot = 1,     // <C, gram> = f_3
};
// EM statistics of a tensor (em)
enum EmStat { kEmNum = 0, kEmDen = 1, kEmObsRes = 2, kEmObsX2 = 3, kEmStats = 4 };
// held-out sums of a tensor (heldout; heldout.h): written only while the tensor has a list attached
enum HeldoutSlot { kHoRes = 0, kHoY2 = 1, kHoM2 = 2, kHoSlots = 4 };
// ranking-metric sums of a tensor (rank; rank_metrics.h): written only while the tensor has a ranking list attached.
// Counts are doubles holding integers.
enum RankSlot {
  kRankN = 0,         // queries with rank >= 0
  kRankNAuc = 1,      // those of them with ncand >= 2
  kRankHits = 2,      // #{rank < k}
  kRankNdcg = 3,      // sum over rank < k of 1 / log2(rank + 2)
  kRankMrr = 4,       // sum of 1 / (rank + 1)
  kRankAuc = 5,       // sum over the kRankNAuc queries of 1 - rank / (ncand - 1)
  kRankUsed = 6,
  kRankSlots = 8,     // two spare
};
// sums per slab in a PARAFAC2 block's q (p2_q)[kSlabSums * k + ...]
enum SlabSum {
  kSlabGapP = 0,      // ||B_k - P_k DeltaB||^2
  kSlabNormB = 1,     // ||B_k||^2
  kSlabGapZ = 2,      // ||B_k - Z_k||^2
  kSlabSmooth = 3,    // ||B_k - B_{k-1}||^2
  kSlabSums = 4,
};

struct ArenaView;

struct ArenaLayout {
  int n_modes = 0, n_tensors = 0, n_couplings = 0;
  std::vector<int> K;             // per tensor: slabs of a PARAFAC2 block, 0 for a CP block
  std::vector<size_t> off_p2;     // per tensor: byte offset of a PARAFAC2 block's res | q | regv
  size_t off_ctl = 0, bytes = 0;

  int n_doubles() const {
    return n_modes * (kSlotsPerMode + kResidPerMode) + (kSlotsPerTensor + kEmStats + kHoSlots + kRankSlots) * n_tensors + kScratchSlots;
  }
  int n_ctl() const { return n_modes + n_couplings; }       // the records the host checks (one spare behind them)
  void build(int modes, int tensors, int couplings, const std::vector<int>& slabs) {
    n_modes = modes; n_tensors = tensors; n_couplings = couplings; K = slabs;
    off_ctl = (size_t)round_up((int64_t)n_doubles() * (int64_t)sizeof(double), 64);
    bytes = (size_t)round_up((int64_t)(off_ctl + (size_t)(n_ctl() + 1) * sizeof(AdmmCtl)), 64);
    off_p2.assign(n_tensors, 0);
    for (int p = 0; p < n_tensors; ++p)
      if (K[p] > 0) { off_p2[p] = bytes; bytes += ((size_t)(2 + kSlabSums) * K[p] + 1) * sizeof(double); }
  }
  inline ArenaView at(void* base) const;
};

struct ArenaView {
  const ArenaLayout* L = nullptr;
  char* base = nullptr;

  double* doubles() const { return reinterpret_cast<double*>(base); }
  double* mode_obj(int m) const { return doubles() + (int64_t)m * kSlotsPerMode; }
  double* tensor_obj(int p) const { return mode_obj(L->n_modes) + kSlotsPerTensor * p; }
  double* resid(int m) const { return tensor_obj(L->n_tensors) + (int64_t)m * kResidPerMode; }
  double* scratch() const { return resid(L->n_modes); }
  double* em(int p) const { return scratch() + kScratchSlots + kEmStats * p; }
  double* heldout(int p) const { return em(L->n_tensors) + kHoSlots * p; }
  double* rank(int p) const { return heldout(L->n_tensors) + kRankSlots * p; }
  AdmmCtl* ctl(int i) const { return reinterpret_cast<AdmmCtl*>(base + L->off_ctl) + i; }
  // PARAFAC2 block p: K + 1 slab residuals (+ the not-PD flag of sharded slabs), kSlabSums K gap sums, K regulariser values
  double* p2_res(int p) const { return reinterpret_cast<double*>(base + L->off_p2[p]); }
  double* p2_q(int p) const { return p2_res(p) + L->K[p] + 1; }
  double* p2_regv(int p) const { return p2_q(p) + (int64_t)kSlabSums * L->K[p]; }
};

inline ArenaView ArenaLayout::at(void* base) const { return ArenaView{this, static_cast<char*>(base)}; }

}  // namespace aoadmm
