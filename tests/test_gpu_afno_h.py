"""rpb_afno_mlp_f16x2 (csrc/rpb_dpot_h.hip): the AFNO block MLP of the opt-in "f16x2" eval arithmetic, out = gelu(X Wa + ba) Wb + bb per
(token, block) with complex weights, against the same formula in fp64 (complex products written out, GELU by erf).

Bound: Rel-L2 < 2e-6, the project's f16x2 kernel bound (tests/test_gpu_gemm3h.py), over the whole output and for the worst token row
on its own -- the case a per-tensor activation scale cannot pass when the tokens are spread over 40 binades.  Shapes: dpot_s's blocks
(8 x 128) with full tiles and a ragged one, dpot_l's (16 x 96) with a ragged tile and a single token.  X and out stand in a guard-banded
arena (tests/guarded.py): the guards around out and X itself are bit-identical after the call, every output element is written.

Measured on an MI355X: 2.4e-7 to 2.8e-7 for random inputs, token scales and the zero token (a single token 1.1e-7 to 2.5e-7), 2.5e-8
for small weights; the worst token row 3.1e-7; every case below half its bound."""
import functools

import pytest
import torch

from conftest import rel_l2
from guarded import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-6
SHAPES = [(144, 8, 128), (50, 16, 96), (1, 16, 96), (33, 8, 128)]
INPUTS = ["random", "token_scales", "zero_token", "w_small"]


@functools.lru_cache(maxsize=None)
def _case(ntok, nb, bs, kind):
    gen = torch.Generator().manual_seed(7 * ntok + nb + bs)
    C = nb * bs
    X = torch.randn(ntok, 2, C, generator=gen)
    w1, w2 = (torch.randn(2, nb, bs, bs, generator=gen) / bs ** 0.5 for _ in range(2))
    b1, b2 = (0.1 * torch.randn(2, nb, bs, generator=gen) for _ in range(2))
    if kind == "token_scales":
        X = X * torch.tensor([2.0 ** ((7 * i) % 41 - 25) for i in range(ntok)]).view(ntok, 1, 1)
    elif kind == "zero_token":
        X = X.clone()
        X[ntok // 2] = 0
    elif kind == "w_small":
        w1, w2 = w1 * 2.0 ** -12, w2 * 2.0 ** -9
    return X, w1, b1, w2, b2, _want(X, w1, b1, w2, b2, nb, bs)


def _want(X, w1, b1, w2, b2, nb, bs):
    ntok = X.shape[0]
    x = X.double().view(ntok, 2, nb, bs)

    def layer(xr, xi, w, b):
        w, b = w.double(), b.double()
        re = torch.einsum("tbi,bio->tbo", xr, w[0]) - torch.einsum("tbi,bio->tbo", xi, w[1]) + b[0]
        im = torch.einsum("tbi,bio->tbo", xr, w[1]) + torch.einsum("tbi,bio->tbo", xi, w[0]) + b[1]
        return re, im

    hr, hi = layer(x[:, 0], x[:, 1], w1, b1)
    g = torch.nn.functional.gelu
    orr, oi = layer(g(hr), g(hi), w2, b2)
    return torch.stack([orr, oi], 1).reshape(ntok, 2, nb * bs)


def _run(X, w1, b1, w2, b2, nb, bs):
    from realpdebench_amd import ops
    ntok = X.shape[0]
    ar = Arena(DEV)
    x_, o_ = ar.inp(X, ld=2 * nb * bs), ar.out(ntok, 2, nb * bs, ld=2 * nb * bs)
    w1z, w2z = ops.afno_wprep_f16x2(w1.to(DEV), nb, bs), ops.afno_wprep_f16x2(w2.to(DEV), nb, bs)
    ops.afno_mlp_f16x2(x_.op, w1z, b1.to(DEV).contiguous(), w2z, b2.to(DEV).contiguous(), o_.op, ntok, nb, bs)
    ar.check()
    return o_.get()


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("ntok,nb,bs", SHAPES)
def test_afno_mlp_f16x2_against_fp64(ntok, nb, bs, kind):
    from realpdebench_amd import ops
    assert ops.afno_f16x2_supported(nb, bs)
    X, w1, b1, w2, b2, want = _case(ntok, nb, bs, kind)
    out = _run(X, w1, b1, w2, b2, nb, bs)
    assert torch.equal(out, _run(X, w1, b1, w2, b2, nb, bs)), "two calls must give bit-equal outputs"
    assert bool(torch.isfinite(out).all())
    e = rel_l2(out, want)
    d = (out.double() - want).view(ntok, -1).norm(dim=1) / want.view(ntok, -1).norm(dim=1)
    er = float(d.max())
    print(f"afno_mlp_f16x2 ntok={ntok} nb={nb} bs={bs} [{kind}]: Rel-L2 {e:.2e}, worst token row {er:.2e} (bound {BOUND:.0e})")
    assert e < BOUND
    assert er < BOUND


def test_afno_f16x2_refuses_unsupported_block_size():
    from realpdebench_amd import _lib, ops
    assert not ops.afno_f16x2_supported(8, 24)
    with pytest.raises(_lib.RpbError):
        ops.afno_wprep_f16x2(torch.zeros(2, 8, 24, 24, device=DEV), 8, 24)
