"""Two fp64 numpy restatements of the reference's DMD forward (realpdebench/model/dmd.py:22-128, 204-209), written from its
formulas: ``direct`` as the reference runs it (SVD of the snapshot matrix, eigen-decomposition of the reduced operator, modes,
``lstsq`` amplitudes, mode selection, the sum over modes), and ``gram`` through the T x T Gram matrix with the rank floor -- the form
the product's host solve and kernels implement.  Neither imports the product."""
import numpy as np

DT = 0.0025
EPS32 = float(np.finfo(np.float32).eps)


def snapshots(x, f):
    """x [T,H,W,C] -> X [T, H W f] in fp64 (rows = frames)."""
    return np.asarray(x, dtype=np.float64)[..., :f].reshape(x.shape[0], -1)


def direct(x, f, n_modes, n_predict):
    """One sample, x [T,H,W,C] -> [n_predict,H,W,f], fp64."""
    X = snapshots(x, f).T                                   # [n, T]
    T = X.shape[1]
    X1, X2 = X[:, :-1], X[:, 1:]
    U, s, Vt = np.linalg.svd(X1, full_matrices=False)
    VS = Vt.T / s
    lam, W = np.linalg.eig(U.T @ X2 @ VS)
    Phi = X2 @ VS @ W
    b = np.linalg.lstsq(Phi, X[:, 0].astype(complex), rcond=EPS32 * max(Phi.shape))[0]     # the cutoff of the reference's complex64 call
    if n_modes is not None and n_modes < len(lam):
        idx = np.argsort(np.abs(b))[::-1][:n_modes]
        Phi, lam, b = Phi[:, idx], lam[idx], b[idx]
    t = (T + np.arange(n_predict)) * DT
    pred = ((Phi * b) @ np.exp(lam[:, None] * t[None, :])).real           # [n, S]
    return pred.T.reshape((n_predict,) + x.shape[1:3] + (f,))


def gram_coefficients(G, n, n_modes, n_predict, floor=2.0 ** -20):
    """G [T,T] -> M [T-1, n_predict] with pred[s] = sum_k M[k,s] X[k+1]."""
    T = G.shape[0]
    s2, V = np.linalg.eigh(G[:-1, :-1])
    s2, V = s2[::-1].clip(min=0), V[:, ::-1]
    s = np.sqrt(s2)
    if s[0] == 0:
        return np.zeros((T - 1, n_predict))
    r = int((s > floor * s[0]).sum())
    VS = V[:, :r] / s[:r]
    lam, W = np.linalg.eig(VS.T @ G[:-1, 1:] @ VS)
    Q = VS @ W
    N = Q.conj().T @ G[1:, 1:] @ Q
    rhs = Q.conj().T @ G[1:, 0]
    mu, Z = np.linalg.eigh((N + N.conj().T) / 2)
    mu = mu.clip(min=0)
    keep = np.sqrt(mu) > EPS32 * max(n, r) * np.sqrt(mu.max())
    b = Z[:, keep] @ ((Z[:, keep].conj().T @ rhs) / mu[keep])
    idx = np.arange(r)
    if n_modes is not None and n_modes < r:
        idx = np.argsort(np.abs(b))[::-1][:n_modes]
    t = (T + np.arange(n_predict)) * DT
    return ((Q[:, idx] * b[idx]) @ np.exp(lam[idx, None] * t[None, :])).real


def gram(x, f, n_modes, n_predict):
    """One sample through the Gram form, fp64."""
    X = snapshots(x, f)
    M = gram_coefficients(X @ X.T, X.shape[1], n_modes, n_predict)
    return (M.T @ X[1:]).reshape((n_predict,) + x.shape[1:3] + (f,))


def batch(fn, x, f, n_modes, n_predict):
    return np.stack([fn(xi, f, n_modes, n_predict) for xi in x])


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def rollout(fn, x, f, n_modes, n_predict, steps, stats, c_out):
    """eval.py:305-321 for a model that predicts ``f`` leading channels, raw data ``x`` [B,T,H,W,C_in], fp64: returns the normalised
    predictions ``[B, steps * T, H, W, f]`` (control channels cut)."""
    mi, mt, si, st = (np.asarray(v, dtype=np.float64) for v in stats)
    x = np.asarray(x, dtype=np.float64)
    para = x[..., c_out:] if x.shape[-1] != c_out else None
    preds = [(x - mi[:x.shape[-1]]) / si[:x.shape[-1]]]
    for _ in range(steps):
        p = batch(fn, preds[-1], f, n_modes, n_predict) * st[:f] + mt[:f]
        if para is not None:
            p = np.concatenate([p, para], -1)
        preds.append((p - mi[:p.shape[-1]]) / si[:p.shape[-1]])
    out = np.concatenate(preds[1:], 1)
    return out[..., :f]
