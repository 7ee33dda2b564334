"""DMD -- the reference's dynamic-mode-decomposition baseline (realpdebench/model/dmd.py) on MI355X.

The reference fits one exact DMD per sample on the host: float32 SVD of the ``[n, T-1]`` snapshot matrix (``n = H W f``), the reduced
operator's eigen-decomposition, a complex ``lstsq`` for the amplitudes, the ``n_modes`` largest of them, and a Python double loop over
modes and steps.  Every one of those quantities is a function of the ``T x T`` Gram matrix ``G = X X^T`` of the input frames, and the
prediction is a linear combination of the frames ``X[1:]`` themselves, so here the device reads the input twice and nothing of size
``n x r`` exists:

    G = ops.dmd_gram(x, f)                          # HIP, fp64 accumulation                 [B, T, T]
    M = dmd_coefficients(G, n, n_modes, n_predict)  # host, numpy fp64, order <= T - 1       [B, T-1, n_predict]
    pred = ops.dmd_predict(x, M, f)                 # HIP, fp64 accumulation, fp32 output    [B, n_predict, H, W, f]

The host solve is deliberate: a nonsymmetric complex eigenproblem of order <= 31 per sample, which the reference solves on the host
too; it costs one ``B T^2`` copy down, one ``B (T-1) S`` copy up and one synchronisation per forward."""
import numpy as np
import torch

from .. import ops
from .model import Model

DT = 0.0025                      # dmd.py:117: the exponent is lambda * t * 0.0025 with lambda itself (not its logarithm); kept
RANK_FLOOR = 2.0 ** -20          # singular values at or below this fraction of the largest are dropped (the one deviation: DESIGN.md 18.2)
T_MAX = S_MAX = 32               # rpb_dmd_gram / rpb_dmd_predict: a 2 x 2 grid of 16 x 16 fp64 MFMA tiles


def _solve_group(G, V, s, r, n, n_modes, n_predict):
    """Samples whose snapshot matrices have the same rank ``r`` after the floor, batched: G [g,T,T], V [g,T-1,T-1] and s [g,T-1]
    (eigenvectors and singular values of G11 in descending order) -> M [g,T-1,n_predict]."""
    T = G.shape[1]
    H = lambda A: A.conj().transpose(0, 2, 1)
    G12, G22, g0 = G[:, :-1, 1:], G[:, 1:, 1:], G[:, 1:, 0]
    VS = V[:, :, :r] / s[:, None, :r]
    lam, W = np.linalg.eig(VS.transpose(0, 2, 1) @ G12 @ VS)      # unit-norm columns, like the reference's call
    Q = VS @ W                                                    # modes Phi = X2 Q are never formed
    N = H(Q) @ G22 @ Q                                            # Phi^H Phi
    rhs = (H(Q) @ g0[:, :, None])[:, :, 0]                        # Phi^H x0
    mu, Z = np.linalg.eigh((N + H(N)) / 2)
    mu = np.maximum(mu, 0.0)
    # lstsq(rcond=None) on complex64: singular values of Phi (sqrt mu) at or below eps32 max(n, r) times the largest are cut
    keep = np.sqrt(mu) > np.finfo(np.float32).eps * max(n, r) * np.sqrt(mu.max(axis=1, keepdims=True))
    coef = np.where(keep, (H(Z) @ rhs[:, :, None])[:, :, 0] / np.where(keep, mu, 1.0), 0.0)
    b = (Z @ coef[:, :, None])[:, :, 0]
    if n_modes is not None and n_modes < r:                       # the n_modes largest |b|; the others contribute nothing
        drop = np.argsort(np.abs(b), axis=1)[:, ::-1][:, n_modes:]
        np.put_along_axis(b, drop, 0.0, axis=1)
    t = (T + np.arange(n_predict)) * DT
    return np.ascontiguousarray(((Q * b[:, None, :]) @ np.exp(lam[:, :, None] * t[None, None, :])).real)


def dmd_coefficients(G, n, n_modes, n_predict):
    """``G`` fp64 ``[B,T,T]`` (Gram matrices of the input frames over ``n`` values each) -> ``M`` fp64 ``[B,T-1,n_predict]`` with
    ``pred[s] = sum_k M[k,s] X[k+1]``: steps 1-6 of DESIGN.md section 18.1, pure numpy; the LAPACK calls are batched over the samples
    that keep the same rank (as a rule, all of them)."""
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 3 or G.shape[1] != G.shape[2] or G.shape[1] < 3:
        raise ValueError(f"dmd_coefficients: G must be [B,T,T] with T >= 3, got {G.shape}")
    n, n_predict = int(n), int(n_predict)
    s2, V = np.linalg.eigh(G[:, :-1, :-1])                        # ascending
    s, V = np.sqrt(np.maximum(s2[:, ::-1], 0.0)), V[:, :, ::-1]
    rank = np.count_nonzero(s > RANK_FLOOR * s[:, :1], axis=1)    # 0 for an all-zero input, which predicts zero
    M = np.zeros((G.shape[0], G.shape[1] - 1, n_predict))
    for r in np.unique(rank[rank > 0]):
        sel = np.flatnonzero(rank == r)
        M[sel] = _solve_group(G[sel], V[sel], s[sel], int(r), n, n_modes, n_predict)
    return M


class DMD(Model):
    """``DMD(n_modes, n_predict, input_feature, n_autoregressive, shape_in, shape_out)``: no parameters, not trained.

    ``forward(x[B,T,H,W,C]) -> [B,n_predict,H,W,f]`` reads the first ``f = input_feature`` channels and predicts those (not ``C``
    channels, as in the reference).  ``ARITHS`` has the default only."""
    ARITHS = ("f32",)
    training_unavailable = ("DMD is not trained: it is fitted to each input inside forward (realpdebench/model/dmd.py); "
                            "DMD on MI355X covers the forward, the rollout and the evaluation loop")
    PREDICTS_LEADING_CHANNELS = True     # rollout / evaluate: the output has input_feature channels, feedback reads only those

    def __init__(self, n_modes, n_predict, input_feature, n_autoregressive, shape_in, shape_out):
        super().__init__()
        self.shape_in, self.shape_out = tuple(shape_in), tuple(shape_out)
        T, C = self.shape_in[0], self.shape_in[-1]
        f = int(input_feature)
        if T > T_MAX:
            raise NotImplementedError(f"DMD on MI355X takes at most {T_MAX} input frames (the Gram kernel's tile grid), got T = {T}")
        if T < 3:
            raise ValueError(f"DMD needs at least 3 input frames (two snapshot pairs), got T = {T}")
        if not 1 <= int(n_predict) <= S_MAX:
            raise NotImplementedError(f"DMD on MI355X predicts 1 to {S_MAX} frames per forward, got n_predict = {n_predict}")
        if not 1 <= f <= C:
            raise ValueError(f"input_feature = {f} must be between 1 and the {C} input channels")
        if n_modes is not None and int(n_modes) < 1:
            raise ValueError(f"n_modes must be None or at least 1, got {n_modes}")
        self.n_modes = None if n_modes is None else int(n_modes)
        self.n_predict, self.input_feature, self.N_autoregressive = int(n_predict), f, n_autoregressive
        self.register_buffer("_anchor", torch.zeros(1), persistent=False)      # follows .to(device): the model has nothing else to move

    @property
    def device(self):
        return self._anchor.device

    @torch.no_grad()
    def forward(self, x):
        self._require_hip(x)
        if x.dim() != 5 or x.shape[1] != self.shape_in[0] or x.shape[-1] < self.input_feature:
            raise ValueError(f"DMD.forward: expected [B,{self.shape_in[0]},H,W,C >= {self.input_feature}], got {tuple(x.shape)}")
        B, T, H, W, C = x.shape
        f = self.input_feature
        x4 = x.detach().contiguous().float().view(B, T, H * W, C)
        G = ops.dmd_gram(x4, f)
        Gh = G.cpu().numpy()                                           # the forward's one synchronisation
        M = dmd_coefficients(Gh, H * W * f, self.n_modes, self.n_predict)
        out = ops.dmd_predict(x4, torch.from_numpy(M).to(x.device), f)
        return out.view(B, self.n_predict, H, W, f)

    def train_loss(self, input, target):
        raise NotImplementedError(self.training_unavailable)

    def load_checkpoint(self, checkpoint_path, device):
        """Opens nothing (the YAMLs carry ``checkpoint_path: 'no model needed'``): the meta entries are all ``None``."""
        from ._common import META_KEYS
        return {meta: None for meta in META_KEYS.values()}
