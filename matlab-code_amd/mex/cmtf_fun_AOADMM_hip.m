function [G,out] = cmtf_fun_AOADMM_hip(Z,Znorm_const,G,fh,gh,lscalar,uscalar,options)
% Drop-in for cmtf_fun_AOADMM (same signature, functions/cmtf_fun_AOADMM.m:1) that runs the
% AO-ADMM outer loop on an MI355X through aoadmm_mex / libaoadmm_hip.so.
%
% Use: in functions/cmtf_AOADMM.m line 193 replace
%        [Fac,out] = cmtf_fun_AOADMM(Z,Znorm_const, G,fh,gh,lscalar,uscalar,options);
%      by
%        [Fac,out] = cmtf_fun_AOADMM_hip(Z,Znorm_const, G,fh,gh,lscalar,uscalar,options);
% Nothing else changes: Z, the 'init' struct, init_options and options keep their fields; optional
% engine settings live in options.hip (device = 0 or devices = [0 1 ... 7] for several GPUs from this one
% MATLAB process, precision = 'f64' | 'f32' | 'f16', par2_slab_sharding, sparse_sharding, sparse_observed_only,
% no_permuted_copy).  sparse_observed_only = 1 (every sparse CP block) or a list of block numbers: the entries an
% sptensor does not store are MISSING, not zero, and are fitted by the EM step as Z.miss does for full data (Z.miss itself
% stays refused for an sptensor, cmtf_AOADMM.m:77-79); not together with sparse_sharding.
% sparse_entry_weights = cell over the blocks, {p} one weight in [0,1] per stored entry of the sptensor Z.object{p}
% (aligned with its subs / vals) or []; sparse_unstored_weight = one number for all named blocks or a cell over the
% blocks: weighted least squares, the unstored entries are zeros of that small confidence.  A named block is
% observed-only as well; weights above 1 are divided by their maximum by the caller; not together with sparse_sharding.
% 'f16': dense 3-way CP blocks without Z.miss are stored as fp16 with one power-of-two scale per block (half the bytes
% of every tensor pass, 6 instead of 16 resident bytes per entry; the model is fitted to the quantised data), every other
% dense block as fp32; not with several devices, not with no_permuted_copy = 1.
%
% Function handles cannot cross to the GPU, so Z.prox_operators / Z.reg_func (cmtf_AOADMM.m:30-32) are
% dropped and the MEX gateway re-reads the constraint descriptors Z.constraints{m}. Sparse CP blocks (an
% sptensor, or a sparse double matrix for a 2-way block) go to the device as they are, as COO nonzeros in fp64;
% so do the slabs of a PARAFAC2 block when every Z.object{p}{k} is a sparse double matrix.
% Models the device path does not cover ('custom' constraints, KL/IS/beta losses) raise cmtf:hip:unsupported,
% which is caught here and handed to the original MATLAB implementation, so every example script keeps running.
% Znorm_const, fh, gh, lscalar, uscalar are only needed by that fallback.

    Zs = Z;
    if isfield(Zs,'prox_operators'), Zs = rmfield(Zs,'prox_operators'); end
    if isfield(Zs,'reg_func'),       Zs = rmfield(Zs,'reg_func');       end
    for p = 1:numel(Zs.object)           % dense Tensor Toolbox objects -> plain double arrays; sptensor and
        if isa(Zs.object{p},'tensor')    % sparse matrices are read by the gateway as they are (no densifying)
            Zs.object{p} = double(Zs.object{p});
        end
    end
    if isfield(Zs,'miss')                % masks (sptensor / logical, cmtf_AOADMM.m:88-119) -> dense uint8, 1 = observed
        for p = 1:numel(Zs.miss)
            if isempty(Zs.miss{p}), continue; end
            if iscell(Zs.miss{p})
                Zs.miss{p} = cellfun(@(m) uint8(m ~= 0), Zs.miss{p}, 'UniformOutput', false);
            else
                Zs.miss{p} = uint8(double(full(Zs.miss{p})) ~= 0);
            end
        end
    end
    try
        tstart = tic;
        if any(strcmp(options.Display,{'iter','final'}))   % header, cmtf_fun_AOADMM.m:44-51
            if isfield(Zs,'miss') && ~isempty(Zs.miss) && any(~cellfun(@isempty,Zs.miss))
                fprintf(1,' Iter  f total      f tensors      f couplings    f constraints    f PAR2 couplings  f_rel_miss\n');
            else
                fprintf(1,' Iter  f total      f tensors      f couplings    f constraints    f PAR2 couplings\n');
            end
            fprintf(1,'------ ------------ -------------  -------------- ---------------- ----------------\n');
        end
        [G,out] = aoadmm_mex(Zs, G, options);   % with Display = 'iter' the gateway prints a row every DisplayIters iterations
        if any(strcmp(options.Display,{'iter','final'}))   % final row, cmtf_fun_AOADMM.m:496-503
            it = out.OuterIterations;
            ft = out.func_val_conv(it+1); fc = out.func_coupl_conv(it+1);
            fz = out.func_constr_conv(it+1); fp = out.func_PAR2_coupl(it+1);
            if isfield(out,'func_rel_missing')
                fprintf(1,'%6d %12f %12f %12f %12f %12f %12f\n', it, ft+fc+fz+fp, ft, fc, fz, fp, out.func_rel_missing(it+1));
            else
                fprintf(1,'%6d %12f %12f %12f %12f %12f\n', it, ft+fc+fz+fp, ft, fc, fz, fp);
            end
        end
        out.wall_time_hip = toc(tstart);
    catch err
        if strcmp(err.identifier,'cmtf:hip:unsupported')
            warning('cmtf:hip:fallback','%s -- running the MATLAB implementation instead.',err.message);
            [G,out] = cmtf_fun_AOADMM(Z,Znorm_const,G,fh,gh,lscalar,uscalar,options);
        else
            rethrow(err);
        end
    end
end
