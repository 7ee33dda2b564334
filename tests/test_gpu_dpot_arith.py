"""DPOT.set_arith("f16x2") on the GPU: the dense products of the eval forward on rpb_gemm3hk (tests/test_gpu_gemm3hk.py) and
rpb_afno_mlp_f16x2 (tests/test_gpu_afno_h.py).  ``DPOT.ALL_F16X2_SITES`` is what is wired, ``DPOT.F16X2_SITES`` the default routing
(DESIGN.md section 14.1); a site whose shape the kernel refuses stays on the default kernel.

Golden case (tests/golden/dpot_small.npz; embed 256, so every token GEMM has K <= 512 and stays on the default kernel: the AFNO MLP is
what moves): against the reference's ``pred`` < 1e-5 (the bound of tests/test_gpu_dpot.py), against the default path < 5e-6 (the
project's model-level f16x2 bound), not bit-equal to it, two calls bit-equal, ``set_arith("f32")`` reproduces the default bits.  The
configurations of ``test_dpot_s_widths_vs_oracle`` and ``test_dpot_l_block_shapes_and_truncated_modes_vs_oracle`` (depth 1) at B = 1 and
2, eval forward against the default path < 5e-6 with the default routing and with every wired site on, and WHICH sites ran on the new
kernels (from the launch labels): mlp0, mlp2, out0 and afno with every site on -- out2 has K = 32 / 64 and tagg K = 256 / 128 there.  The
sliding-window and resize fixtures against the default path; the planes follow an in-place weight change and a ``load_state_dict``
performed in "f16x2" mode; ``train_loss`` + backward are bit-equal under either setting; the eval entry point.

Measured on an MI355X (each test prints its figure; profiles/dpot_arith_probe.txt holds the probe's output at the cylinder configs):
golden eval against the default path 4.4e-7, against the reference's vector 6.5e-7 (default path 6.6e-7); dpot_s geometry 9.2e-8, dpot_l
geometry 1.2e-7 (B = 1 and 2 alike); sliding windows 2.0e-7, resize 1.7e-7; after the in-place changes and ``load_state_dict`` 1.1e-7 to
1.3e-7; the full-depth dpot_l forward in the probe 1.0e-6.  Every listed case is below half its bound."""
import os

import pytest
import torch
import yaml

from conftest import ROOT, dpot_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 5e-6
CFG_S = dict(img_size=128, in_channels=4, out_channels=4, in_timesteps=4, out_timesteps=4, patch_size=8, embed_dim=1024, depth=1,
             n_blocks=8, modes=32, mlp_ratio=1, out_layer_dim=32, n_cls=12, time_agg="exp_mlp")
CFG_L = dict(img_size=64, in_channels=4, out_channels=4, in_timesteps=2, out_timesteps=2, patch_size=8, embed_dim=1536, depth=1,
             n_blocks=16, modes=3, mlp_ratio=4, out_layer_dim=64, n_cls=12, time_agg="mlp")


def _golden_model(g, **over):
    from realpdebench_amd.model.dpot import DPOT
    cfg = {k: v for k, v in g["cfg"].items() if k not in ("data_out_channels",)}
    cfg.update(over)
    m = DPOT(shape_in=tuple(g["x"].shape[1:]), shape_out=tuple(g["y"].shape[1:]), normalize=False, act="gelu", **cfg).cuda()
    missing, unexpected = m.load_state_dict(g["sd"], strict=True)
    assert not missing and not unexpected
    return m


def _random_model(cfg, S, Cd, seed):
    """Random weights of the model's own initialisation, perturbed so that every bias / affine matters (tests/test_gpu_dpot.py)"""
    from realpdebench_amd.model.dpot import DPOT
    torch.manual_seed(seed)
    m = DPOT(shape_in=(cfg["in_timesteps"], S, S, Cd), shape_out=(cfg["out_timesteps"], S, S, Cd), normalize=False, act="gelu", **cfg)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "norm" in n or n.endswith("bias") or "pos_embed" in n:
                p.add_(0.1 * torch.randn_like(p))
            if n.endswith((".b1", ".b2", ".w1", ".w2")):
                p.copy_(torch.randn_like(p) / p.shape[-1] ** 0.5)
    return m.cuda().eval()


def _labels(fn):
    """fn() with the launch bookkeeping on: (its value, the labels of the launches it made)"""
    from realpdebench_amd import _lib
    old = _lib.PROFILE
    _lib.PROFILE = {}
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, set(_lib.PROFILE)
    finally:
        _lib.PROFILE = old


def test_golden_eval_f16x2_matches_reference_and_default():
    g = dpot_golden()
    m = _golden_model(g).eval()
    x = g["x"].cuda()
    assert m.arith == "f32"
    with torch.no_grad():
        out0 = m(x)
        assert m.set_arith("f16x2") is m
        out = m(x)
        assert torch.equal(m(x), out), "two f16x2 calls must give bit-equal outputs"
        assert torch.equal(m.set_arith("f32")(x), out0), "set_arith('f32') must reproduce the default output bit for bit"
    e, e0, d = rel_l2(out.cpu(), g["pred"]), rel_l2(out0.cpu(), g["pred"]), rel_l2(out.cpu(), out0.cpu())
    print(f"golden eval: f16x2 against the reference {e:.2e} (default path {e0:.2e}, tol 1e-5), against the default path {d:.2e} (bound 5e-6)")
    assert out.shape == g["pred"].shape and bool(torch.isfinite(out).all())
    assert not torch.equal(out, out0), "the switch must reach the kernels"
    assert e < 1e-5
    assert d < BOUND


@pytest.mark.parametrize("every_site", [False, True], ids=["default_sites", "every_site"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", ["dpot_s", "dpot_l"])
def test_config_geometries_against_default_path(name, B, every_site):
    from realpdebench_amd.model.dpot import DPOT
    cfg, S, Cd, seed = (CFG_S, 128, 2, 5) if name == "dpot_s" else (CFG_L, 64, 3, 6)
    m = _random_model(cfg, S, Cd, seed)
    if every_site:
        m.F16X2_SITES = DPOT.ALL_F16X2_SITES                       # this instance only
    x = torch.randn(B, cfg["in_timesteps"], S, S, Cd, device=DEV)
    with torch.no_grad():
        out0, lab0 = _labels(lambda: m(x))
        out, lab = _labels(lambda: m.set_arith("f16x2")(x))
    d = rel_l2(out.cpu(), out0.cpu())
    print(f"{name} geometry B={B} sites={m.F16X2_SITES}: f16x2 against the default path {d:.2e} (bound 5e-6); ran {m.f16x2_ran}")
    assert not any(l.startswith(("gemm3hk", "afno_mlp_f16x2")) for l in lab0), "the default path must not touch the new kernels"
    E, hid, NU = cfg["embed_dim"], int(cfg["embed_dim"] * cfg["mlp_ratio"]), 64 * cfg["out_layer_dim"]
    site_label = {"mlp0": f"gemm3hk[N{hid},K{E}]", "mlp2": f"gemm3hk[N{E},K{hid}]", "out0": f"gemm3hk[N{NU},K{E}]", "afno": "afno_mlp_f16x2"}
    want = tuple(s for s in ("mlp0", "mlp2", "out0", "afno") if s in m.F16X2_SITES)       # out2 and tagg: K <= 512 at these geometries
    assert m.f16x2_ran == want
    new = {l for l in lab if l.startswith(("gemm3hk[", "afno_mlp_f16x2"))}
    assert new == {site_label[s] for s in want}, new
    assert bool(torch.isfinite(out).all())
    if want:
        assert not torch.equal(out, out0)
    assert d < BOUND


@pytest.mark.parametrize("name", ["dpot_sliding_small", "dpot_resize_small"])
def test_sliding_window_and_resize_fixtures(name):
    g = dpot_golden(name)
    m = _golden_model(g).eval()
    x = g["x"].cuda()
    with torch.no_grad():
        out0 = m(x)
        out = m.set_arith("f16x2")(x)
    d, e = rel_l2(out.cpu(), out0.cpu()), rel_l2(out.cpu(), g["pred"])
    print(f"{name}: f16x2 against the default path {d:.2e} (bound 5e-6), against the reference {e:.2e}; ran {m.f16x2_ran}")
    assert out.shape == g["pred"].shape
    assert not torch.equal(out, out0)
    assert d < BOUND


def test_planes_follow_in_place_changes_and_load_state_dict():
    """dpot_s widths: FeedForward and out0 on rpb_gemm3hk, AFNO on its twin -- all of them from cached planes"""
    from realpdebench_amd.model.dpot import DPOT
    m = _random_model(CFG_S, 128, 2, 5).set_arith("f16x2")
    m.F16X2_SITES = DPOT.ALL_F16X2_SITES
    x = torch.randn(1, 4, 128, 128, 2, device=DEV)
    blk = m.dpot_model.blocks[0]
    with torch.no_grad():
        old = m(x)
        blk.mlp[0].weight.mul_(1.25)                                 # in place: same storage, new version
        out = m(x)
        want = m.set_arith("f32")(x)
        m.set_arith("f16x2")
        blk.filter.w1.mul_(0.75)
        m.dpot_model.out_layer[0].weight.mul_(1.25)
        out1 = m(x)
        want1 = m.set_arith("f32")(x)
        sd2 = {k: v.clone() for k, v in m.state_dict().items()}
        for k in ("dpot_model.blocks.0.mlp.2.weight", "dpot_model.blocks.0.filter.w2", "dpot_model.blocks.0.mlp.0.bias"):
            sd2[k] = sd2[k] * 0.75
        m.set_arith("f16x2").load_state_dict(sd2)
        assert m.arith == "f16x2"
        out2 = m(x)
        want2 = m.set_arith("f32")(x)
    d, d1, d2 = rel_l2(out.cpu(), want.cpu()), rel_l2(out1.cpu(), want1.cpu()), rel_l2(out2.cpu(), want2.cpu())
    print(f"after mlp0.weight.mul_: {d:.2e}; after w1.mul_ and out0.weight.mul_: {d1:.2e}; after load_state_dict in f16x2 mode: {d2:.2e} "
          "(against the default path, bound 5e-6)")
    assert not torch.equal(out, old) and not torch.equal(out1, out) and not torch.equal(out2, out1)
    assert d < BOUND and d1 < BOUND and d2 < BOUND


def test_training_step_is_untouched_by_set_arith():
    g = dpot_golden()
    x, y = g["x"].cuda(), g["y"].cuda()
    res = []
    for arith in ("f32", "f16x2"):
        m = _golden_model(g).train().set_arith(arith)
        loss = m.train_loss(x, y)
        loss.backward()
        res.append((loss.detach(), {n: p.grad for n, p in m.named_parameters()}))
    (l0, g0), (l1, g1) = res
    assert torch.equal(l0, l1)
    assert sum(v is not None for v in g0.values()) > 10
    for n in g0:
        assert (g0[n] is None and g1[n] is None) or torch.equal(g0[n], g1[n]), n


class One(torch.utils.data.Dataset):
    """A one-sample dataset of the given shapes: what ``load_model`` reads its shapes from."""

    def __init__(self, shape_in, shape_out):
        self.s = (torch.zeros(*shape_in), torch.zeros(*shape_out))

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.s


def test_eval_entrypoint_takes_eval_arith_dpot(tmp_path):
    """`python -m realpdebench_amd.eval` with `eval_arith: f16x2` on a small synthetic DPOT YAML: the metrics agree with the default
    arithmetic's to 1e-4 relative; a value the model rejects ends the run with its ValueError (a non-zero exit of the command)."""
    from realpdebench_amd import eval as ev
    from realpdebench_amd.model import load_model
    with open(os.path.join(ROOT, "realpdebench_amd", "configs", "cylinder", "dpot_s.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    shape = [4, 32, 32, 2]
    cfg.update(exp_name="t", results_path=str(tmp_path), shape_in=shape, shape_out=shape, n_train=4, n_val=4, img_size=32, embed_dim=128,
               depth=2, in_timesteps=4, out_timesteps=4, is_use_tb=None, train_batch_size=2, test_batch_size=2, num_update=100)
    torch.manual_seed(0)
    m = load_model(One(shape, shape), device="cpu", **cfg)
    ck = str(tmp_path / "model_0.pth")
    torch.save({"model_state_dict": {k: v.cpu() for k, v in m.state_dict().items()}, "train_losses": [1.0], "val_losses": {}, "iteration": 7,
                "best_iteration": 7, "best_val_loss": 0.5}, ck)             # the reference's format (train.py)
    path = tmp_path / "dpot.yaml"
    path.write_text(yaml.safe_dump(cfg))
    base = ev.main(["--config", str(path), "--checkpoint_path", ck])
    path2 = tmp_path / "dpot_f16x2.yaml"
    path2.write_text(yaml.safe_dump(dict(cfg, eval_arith="f16x2")))
    fast = ev.main(["--config", str(path2), "--checkpoint_path", ck])
    assert set(base) == set(fast)
    n = 0
    for k in base:
        if not isinstance(base[k], (int, float)):
            assert base[k] == fast[k]
            continue
        a, b = float(base[k]), float(fast[k])
        if a == a and b == b:
            assert abs(a - b) <= 1e-4 * max(abs(a), 1e-12), (k, a, b)
            n += 1
    assert n >= 5
    path3 = tmp_path / "bad.yaml"
    path3.write_text(yaml.safe_dump(dict(cfg, eval_arith="fp8")))
    with pytest.raises((ValueError, SystemExit)) as exc:
        ev.main(["--config", str(path3), "--checkpoint_path", ck])
    assert not (isinstance(exc.value, SystemExit) and exc.value.code in (0, None))
