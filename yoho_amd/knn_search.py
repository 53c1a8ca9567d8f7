"""utils/knn_search.py mirror: brute-force nearest neighbours on the GPU (yoho_nn_search, yoho_knn_search).

``knn_module.KNN(1)(target_F (1,f,n), source_F (1,f,m)) -> (d (1,1,m), idx (1,1,m))`` as the reference (the only
form the YOHO pipeline itself builds: tests/matcher.py:17, YOHO_testset.py:66).

``knn_module.KNN(k)`` with 2 <= k <= 16 is the reference's ``find_knn_gpu`` branch (utils/knn_search.py:68-106,
155-162): ``find_knn_gpu(source_F, target_F) -> (dists (N,1,k), inds (N,k))`` and
``KNN(k)(target_F, source_F) -> (d (1,k,1,m), idx (1,k,m))``, host tensors, every row ascending by (distance, target
index) - ``torch.topk(-dist, k)``'s answer wherever the k + 1 smallest distances of a row are distinct (torch leaves
the order of equal values open; here the lower index comes first).  k > 16 raises NotImplementedError, k beyond the
number of targets RuntimeError as ``torch.topk`` does."""
import numpy as np
import torch

from . import hip


class modified_knn_matcher():
    def __init__(self, k=1):
        self.k = k
        self.ctx = hip.get_context()

    def _prep(self, F):
        F = F.squeeze()
        if F.dim() == 1:
            F = F[None]
        return F.to(device="cuda", dtype=torch.float32).contiguous()

    def find_nn_gpu(self, source_F, target_F, nn_max_n=1000, return_distance=True, dist_type='SquareL2'):
        """utils/knn_search.py:26-66.  Returns (dists, inds) - in that order, as the reference."""
        if dist_type not in ("L2", "SquareL2"):
            raise NotImplementedError('Not implemented')
        F0, F1 = self._prep(source_F), self._prep(target_F)
        if F0.shape[1] not in (3, 32):
            raise NotImplementedError(f"feature width {F0.shape[1]} (the path uses 32-D descriptors and 3-D points)")
        d, inds = self.ctx.nn_search(F0, F1, want_dist=True, squared=(dist_type == "SquareL2"))
        dists, inds = d.cpu(), inds.cpu()
        return (dists, inds) if return_distance else inds

    def find_knn_gpu(self, source_F, target_F, nn_max_n=1000, return_distance=True, dist_type='SquareL2'):
        """utils/knn_search.py:68-106.  Returns (dists (N,1,k), inds (N,k)) - the reference's unsqueeze(1) is kept; nn_max_n (its
        chunk size against memory) is accepted and ignored, as in find_nn_gpu."""
        if dist_type not in ("L2", "SquareL2"):
            raise NotImplementedError('Not implemented')
        if self.k > hip.KNN_MAX:
            raise NotImplementedError(f"k = {self.k}: yoho_knn_search selects at most YOHO_KNN_MAX = {hip.KNN_MAX} neighbours")
        F0, F1 = self._prep(source_F), self._prep(target_F)
        if F0.shape[1] not in (3, 32):
            raise NotImplementedError(f"feature width {F0.shape[1]} (the path uses 32-D descriptors and 3-D points)")
        if self.k > F1.shape[0]:
            raise RuntimeError(f"selected index k out of range: k = {self.k} of {F1.shape[0]} targets")
        d, inds = self.ctx.knn_search(F0, F1, self.k, want_dist=return_distance, squared=(dist_type == "SquareL2"))
        inds = inds.cpu()
        return (d.cpu().unsqueeze(1), inds) if return_distance else inds

    def find_corr(self, F0, F1, subsample_size=-1, mutual=True, nn_max_n=500):
        """utils/knn_search.py:106-136"""
        inds0, inds1 = np.arange(F0.shape[0]), np.arange(F1.shape[0])
        if subsample_size > 0:
            N0, N1 = min(len(F0), subsample_size), min(len(F1), subsample_size)
            inds0 = np.random.choice(len(F0), N0, replace=False)
            inds1 = np.random.choice(len(F1), N1, replace=False)
            F0, F1 = F0[inds0], F1[inds1]
        if not mutual:
            nn = self.find_nn_gpu(F0, F1, return_distance=False).numpy()
            return inds0, inds1[nn]
        m = self.ctx.mutual_nn(self._prep(F0), self._prep(F1)).cpu().numpy()
        return inds0[m[:, 0]], inds1[m[:, 1]]

    def __call__(self, target_F, source_F, nn_max_n=500, dist_type='L2'):
        """utils/knn_search.py:138-162: target_F 1*f*n, source_F 1*f*m -> d, idx of shape 1*1*m (k < 2) or, for k >= 2, what the
        reference's `d.T[None], idx.T[None]` gives on its (m,1,k) / (m,k) tensors: (1,k,1,m) and (1,k,m)."""
        tgt = target_F.squeeze().T
        src = source_F.squeeze().T
        if self.k >= 2:
            d, idx = self.find_knn_gpu(source_F=src, target_F=tgt, nn_max_n=nn_max_n, return_distance=True, dist_type=dist_type)
            return d.permute(2, 1, 0)[None], idx.permute(1, 0)[None]          # .T reverses the dimensions; on 3-D tensors torch deprecates it
        d, idx = self.find_nn_gpu(source_F=src, target_F=tgt, nn_max_n=nn_max_n, return_distance=True, dist_type=dist_type)
        return d[None, None], idx[None, None]


class knn_module_class():
    def KNN(self, k):
        return modified_knn_matcher(k)


knn_module = knn_module_class()
