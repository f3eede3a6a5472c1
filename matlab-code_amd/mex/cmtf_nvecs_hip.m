function U = cmtf_nvecs_hip(Z,n,r,method)
% Drop-in for cmtf_nvecs (functions/cmtf_nvecs.m:1).  Dense data: the I_n x I_n Gram matrix Y = A*A' of the
% mode-n unfolding (cmtf_nvecs.m:40-56) is computed on the MI355X through aoadmm_mex('unfold_gram',...), the
% r leading eigenvectors are taken with eigs exactly as in the reference (:58).
% Sparse data (sptensor / sparse matrix): method 'gram' = the reference's host path, 'iterative' = subspace iteration
% on the nonzeros on the device, aoadmm_mex('nvecs',...), no Gram matrix; omitted or []: 'iterative' for a mode of
% more than 16384 rows, 'gram' otherwise (init_options.nvecs_method of the Python driver).
% Use: in functions/init_coupled_AOADMM_CMTF.m line 52 call cmtf_nvecs_hip instead of cmtf_nvecs.
    P = length(Z.object);
    for p = 1:P
        i = find(Z.modes{p} == n);
        if isempty(i), continue; end
        if nargin < 4, method = []; end
        if ~isempty(method) && ~any(strcmp(method,{'gram','iterative'}))
            error('cmtf:hip:usage','nvecs method must be ''gram'' or ''iterative''');
        end
        if isa(Z.object{p},'sptensor') || issparse(Z.object{p})
            if isempty(method)
                if Z.size{n} > 16384, method = 'iterative'; else, method = 'gram'; end
            end
            if strcmp(method,'iterative')
                U = aoadmm_mex('nvecs', Z.object{p}, i(1), r);
            else
                U = cmtf_nvecs(Z,n,r);      % sparse unfolding: its Gram matrix on the host (sptenmat, cmtf_nvecs.m:41-42)
            end
            return
        end
        if strcmp(method,'iterative')
            error('cmtf:hip:usage','nvecs method ''iterative'' handles sparse data only');
        end
        Y = aoadmm_mex('unfold_gram', double(Z.object{p}), i(1));
        [U,~] = eigs(Y, r, 'LM');
        return
    end
    error('cmtf:hip:usage','mode %d belongs to no data set', n);
end
