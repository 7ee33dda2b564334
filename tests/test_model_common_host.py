"""Host side of realpdebench_amd/model/_common.py (no GPU needed): the invalidation rule of ``LayoutCache``, the stale-layout case it
closes in Transolver._conv_cat (``p.data = other`` leaves ``p._version`` unchanged), ``HipFunction`` on a pure-torch
model, and the arithmetic protocol of ``Model`` (model/model.py): the routing rule of ``_dense`` on recording stand-ins for the ``ops``
names it calls, and ``set_arith`` on all eight model classes."""
import gc
import weakref

import pytest
import torch
import torch.nn as nn

from realpdebench_amd.model._common import HipFunction
from realpdebench_amd.model.model import Model


class _Lin(Model):
    """y = x W^T + b with a CPU ``_forward_hip`` / ``_backward_hip`` pair; ``unused`` never receives a gradient."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.weight = nn.Parameter(torch.randn(3, 5, generator=g))
        self.bias = nn.Parameter(torch.randn(3, generator=g))
        self.unused = nn.Parameter(torch.zeros(2))
        self.builds = 0
        self.state_refs = []

    def layout(self, extra=None):
        def build():
            self.builds += 1
            return self.weight.detach().t().contiguous()

        return self._layouts.get("wt", (self.weight,), build, extra=extra)

    def _forward_hip(self, x, save=None):
        if save is not None:
            save["x"] = x.clone()
            self.state_refs.append(weakref.ref(save["x"]))
        return x @ self.weight.detach().t() + self.bias.detach()

    def _backward_hip(self, sv, g, need_gx=False):
        grads = {self.weight: g.t() @ sv["x"], self.bias: g.sum(0)}
        if need_gx:
            grads["__x__"] = g @ self.weight.detach()
        return grads

    def forward(self, x):
        return HipFunction.apply(x, self, *self.parameters())


# ---------------------------------------------------------------------------------------------------------------- LayoutCache
def test_layout_cache_hits_while_the_sources_are_unchanged():
    m = _Lin()
    a = m.layout()
    assert m.layout() is a and m.builds == 1
    assert torch.equal(a, m.weight.detach().t())


def test_layout_cache_misses_after_an_in_place_update():
    m = _Lin()
    m.layout()
    with torch.no_grad():
        m.weight.copy_(torch.ones(3, 5))
    assert torch.equal(m.layout(), torch.ones(5, 3)) and m.builds == 2


def test_layout_cache_misses_after_a_rebind_and_holds_the_old_tensor():
    m = _Lin()
    m.layout()
    old_ptr, old_version, old_values = m.weight.data_ptr(), m.weight._version, m.weight.detach().clone()
    m.weight.data = torch.full((3, 5), 2.0)
    assert m.weight._version == old_version                       # the hole a version-only key leaves open
    gc.collect()
    held = m._layouts._entries["wt"][2][0]                        # the entry keeps the tensor it was built from: its address cannot be
    assert held.data_ptr() == old_ptr and torch.equal(held, old_values)      # handed to a new tensor while the entry lives
    assert m.weight.data_ptr() != old_ptr
    assert torch.equal(m.layout(), torch.full((5, 3), 2.0)) and m.builds == 2


def test_layout_cache_misses_after_load_state_dict_with_equal_shapes():
    m = _Lin()
    m.layout()
    m.load_state_dict(_Lin().state_dict())                        # the same values, even: the token alone invalidates
    m.layout()
    assert m.builds == 2


def test_layout_cache_misses_after_apply():
    m = _Lin()
    w = m.weight.detach().clone()
    m.layout()
    m.double().float()
    assert torch.equal(m.layout(), w.t()) and m.builds == 2


def test_layout_cache_misses_on_another_extra_key():
    m = _Lin()
    m.layout(extra="f32")
    m.layout(extra="f32")
    assert m.builds == 1
    m.layout(extra="f16x2")
    assert m.builds == 2
    m.layout(extra="f32")                                         # one entry per key: the other arithmetic's layout was dropped
    assert m.builds == 3


# ---------------------------------------------------------------------------------------------------------------- stale layouts
def test_transolver_conv_cat_follows_a_rebound_parameter():
    from realpdebench_amd.model.transolver import Transolver
    m = Transolver(space_dim=3, n_layers=1, n_hidden=64, n_head=2, fun_dim=0, out_dim=3, slice_num=16, mlp_ratio=2, H=8, W=6, D=4)
    w0, b0 = (t.clone() for t in m._conv_cat(0))
    a = m.blocks[0].Attn
    a.in_project_x.weight.data = a.in_project_x.weight.data + 1
    a.in_project_fx.bias.data = a.in_project_fx.bias.data + 1
    w1, b1 = m._conv_cat(0)
    C = m.n_hidden
    assert torch.equal(w1[:C], w0[:C]) and torch.equal(w1[C:], w0[C:] + 1)          # rows C..2C-1 = in_project_x
    assert torch.equal(b1[:C], b0[:C] + 1) and torch.equal(b1[C:], b0[C:])          # entries 0..C-1 = in_project_fx


# ---------------------------------------------------------------------------------------------------------------- HipFunction
@pytest.mark.parametrize("x_grad", [False, True])
def test_hip_function_routes_gradients_and_releases_the_state(x_grad):
    m = _Lin()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 5, generator=g).requires_grad_(x_grad)
    t = torch.randn(4, 3, generator=g)
    ((m(x) - t) ** 2).mean().backward()
    w, b, xr = (v.detach().clone().requires_grad_(True) for v in (m.weight, m.bias, x))
    ((xr @ w.t() + b - t) ** 2).mean().backward()
    assert torch.allclose(m.weight.grad, w.grad, rtol=1e-6, atol=1e-7) and m.weight.grad.shape == m.weight.shape
    assert torch.allclose(m.bias.grad, b.grad, rtol=1e-6, atol=1e-7) and m.bias.grad.shape == m.bias.shape
    assert m.unused.grad is None                                   # absent from the dict
    if x_grad:
        assert torch.allclose(x.grad, xr.grad, rtol=1e-6, atol=1e-7)
    else:
        assert x.grad is None
    gc.collect()
    assert len(m.state_refs) == 1 and m.state_refs[0]() is None     # the saved activations went with the backward call


def test_hip_function_keeps_the_state_until_backward():
    m = _Lin()
    y = m(torch.ones(2, 5))
    gc.collect()
    assert m.state_refs[0]() is not None
    y.sum().backward()
    gc.collect()
    assert m.state_refs[0]() is None


# ---------------------------------------------------------------------------------------------------------------- the routed dense product
class _Routed(Model):
    ALL_F16X2_SITES = F16X2_SITES = ("a", "b")
    F16X2_GEMM = ("gemm3h_supported", "gemm_nt_f16x2")

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.arange(12.0).view(3, 4))


class _Ops:
    """Recording stand-ins for the four ``ops`` names ``Model._dense`` calls; ``supported`` is what the shape predicate answers."""

    def __init__(self, monkeypatch, supported=True):
        from realpdebench_amd import ops
        self.default, self.routed, self.preps, self.asked = [], [], [], []
        monkeypatch.setattr(ops, "gemm_nt", lambda *a, **kw: self.default.append((a, kw)))
        monkeypatch.setattr(ops, "gemm_nt_f16x2", lambda *a, **kw: self.routed.append((a, kw)))
        monkeypatch.setattr(ops, "gemm3h_supported", lambda M, N, K: self.asked.append((M, N, K)) or supported)
        monkeypatch.setattr(ops, "gemm3h_wprep", lambda W: self.preps.append(W) or ("planes", len(self.preps)))
        # the other kernel pair must never be reached from this class
        monkeypatch.setattr(ops, "gemm_nt_f16x2k", lambda *a, **kw: pytest.fail("gemm_nt_f16x2k"))
        monkeypatch.setattr(ops, "gemm3hk_supported", lambda *a, **kw: pytest.fail("gemm3hk_supported"))


A, OUT, BIAS, RES = (torch.full((1,), float(i)) for i in range(4))     # identities are what the fakes compare


def _same(got, want):
    return len(got) == len(want) and all(g is w for g, w in zip(got, want))


@pytest.mark.parametrize("ran_is_none", [True, False])
def test_dense_default_arithmetic_gets_every_argument(monkeypatch, ran_is_none):
    """``ran is None`` is every forward but the f16x2 evaluation one; a site outside ``F16X2_SITES`` under it behaves the same."""
    k, m = _Ops(monkeypatch), _Routed()
    m.F16X2_SITES = ()
    ran = None if ran_is_none else []
    W = m.w.data
    got = m._dense(ran, "a", "a", [m.w], W, A, OUT, 7, 3, 4, bias=BIAS, act=1, residual=RES, pre_out=None, mask=None, drop=None)
    assert got is W and not k.routed and not k.preps and not ran
    (args, kw), = k.default
    assert _same(args[:3], (A, W, OUT)) and args[3:] == (7, 3, 4)
    assert kw == dict(bias=BIAS, act=1, residual=RES, pre_out=None, mask=None, drop=None) and kw["bias"] is BIAS and kw["residual"] is RES


def test_dense_routed_runs_the_f16x2_kernel_once_and_records_the_site(monkeypatch):
    k, m = _Ops(monkeypatch), _Routed()
    ran = []
    got = m._dense(ran, "a", "a", [m.w], m.w.data, A, OUT, 7, 3, 4, bias=BIAS, act=3, residual=RES, mask=None, drop=None, pre_out=None)
    assert got is None and ran == ["a"] and not k.default and k.asked == [(7, 3, 4)]
    (args, kw), = k.routed
    assert _same(args[:1], (A,)) and args[1] == ("planes", 1) and args[2] is OUT and args[3:] == (7, 3, 4)
    assert kw == dict(bias=BIAS, act=3, residual=RES) and kw["bias"] is BIAS and kw["residual"] is RES
    assert len(k.preps) == 1 and torch.equal(k.preps[0], m.w.data)


def test_dense_planes_are_cached_until_a_source_changes(monkeypatch):
    k, m = _Ops(monkeypatch), _Routed()
    fwd = lambda: m._dense([], "a", "a", [m.w], lambda: m.w.data, A, OUT, 7, 3, 4)
    fwd(), fwd()
    assert len(k.preps) == 1 and len(k.routed) == 2
    with torch.no_grad():
        m.w.add_(1.0)                                              # in place
    fwd(), fwd()
    assert len(k.preps) == 2 and torch.equal(k.preps[1], torch.arange(12.0).view(3, 4) + 1)
    m.w.data = torch.zeros(3, 4)                                   # rebound: same _version
    fwd(), fwd()
    assert len(k.preps) == 3 and torch.equal(k.preps[2], torch.zeros(3, 4))
    m.load_state_dict(_Routed().state_dict())
    fwd(), fwd()
    assert len(k.preps) == 4 and torch.equal(k.preps[3], torch.arange(12.0).view(3, 4))
    assert k.routed[-1][0][1] == ("planes", 4) and len(k.routed) == 8 and not k.default


@pytest.mark.parametrize("why", ["site", "predicate", "mask", "drop", "pre_out"])
def test_dense_each_condition_alone_keeps_the_default_kernel(monkeypatch, why):
    k, m = _Ops(monkeypatch, supported=why != "predicate"), _Routed()
    if why == "site":
        m.F16X2_SITES = ("b",)
    only = dict(mask=None, drop=None, pre_out=None)
    if why in only:
        only[why] = (5, 0.5) if why == "drop" else torch.ones(1)
    ran = []
    W = m.w.data
    assert m._dense(ran, "a", "a", [m.w], W, A, OUT, 7, 3, 4, bias=BIAS, **only) is W
    assert ran == [] and not k.routed and not k.preps
    (args, kw), = k.default
    assert _same(args[:3], (A, W, OUT)) and args[3:] == (7, 3, 4)
    assert kw == dict(bias=BIAS, act=0, residual=None, **only) and all(kw[n] is only[n] for n in only)
    assert m._routed_planes(ran, "a", "a", [m.w], W, 7, 3, 4, **only) is None and not k.preps


def test_dense_callable_weight_is_formed_only_where_it_is_read(monkeypatch):
    k, m = _Ops(monkeypatch), _Routed()
    calls = []

    def weight():
        calls.append(1)
        return m.w.data * 2

    ran = []
    assert m._dense(ran, "a", "a", [m.w], weight, A, OUT, 7, 3, 4) is None and len(calls) == 1      # the cache miss: once, for the planes
    assert m._dense(ran, "a", "a", [m.w], weight, A, OUT, 7, 3, 4) is None and len(calls) == 1      # the hit: not at all
    assert ran == ["a", "a"] and len(k.preps) == 1
    W = m._dense(None, "a", "a", [m.w], weight, A, OUT, 7, 3, 4)                                   # the default path: once, and handed back
    assert len(calls) == 2 and torch.equal(W, m.w.data * 2) and k.default[0][0][1] is W and len(k.preps) == 1


# ---------------------------------------------------------------------------------------------------------------- set_arith
def _model_classes():
    from realpdebench_amd.model.cno import CNO3d
    from realpdebench_amd.model.deeponet import DeepONet
    from realpdebench_amd.model.dpot import DPOT
    from realpdebench_amd.model.fno import FNO3d
    from realpdebench_amd.model.galerkin_transformer import GalerkinTransformer3d
    from realpdebench_amd.model.mwt import MWT3d
    from realpdebench_amd.model.transolver import Transolver
    from realpdebench_amd.model.unet import Unet3d
    return FNO3d, Unet3d, Transolver, DPOT, GalerkinTransformer3d, MWT3d, CNO3d, DeepONet


@pytest.mark.parametrize("i", range(8))
def test_set_arith_is_one_switch_on_every_model(i):
    cls = _model_classes()[i]
    three = cls.__name__ == "MWT3d"
    assert issubclass(cls, Model) and cls.ARITHS == (("f32", "bf16x3", "f16x2") if three else ("f32", "f16x2")) and cls.arith == "f32"
    assert [c.__name__ for c in cls.__mro__ if "set_arith" in vars(c)] == {"FNO3d": ["FNO3d", "Model"], "Unet3d": ["Unet3d", "Model"]}.get(
        cls.__name__, ["Model"])
    m = cls.__new__(cls)                                           # bare: the switch needs nothing a constructor builds ...
    if cls.__name__ == "FNO3d":
        m.width, m.modes3, m._ws = 64, 16, {}                      # ... but FNO3d's shape precondition and its workspaces
    text = "arith must be 'f32', 'bf16x3' or 'f16x2', got 'x'" if three else "arith must be 'f32' or 'f16x2', got 'x'"
    with pytest.raises(ValueError) as e:
        m.set_arith("x")
    assert str(e.value) == text and m.arith == "f32"
    for a in cls.ARITHS[::-1]:
        assert m.set_arith(a) is m and m.arith == a


def test_fno_set_arith_keeps_its_own_refusals():
    from realpdebench_amd.model.fno import FNO3d
    m = FNO3d.__new__(FNO3d)
    m.width, m.modes3, m._ws = 32, 4, {(1, False): "eval", (1, True): "train"}
    with pytest.raises(ValueError) as e:                           # an unknown name first, then the shape
        m.set_arith("x")
    assert str(e.value) == "arith must be 'f32' or 'f16x2', got 'x'"
    with pytest.raises(NotImplementedError) as e:
        m.set_arith("f16x2")
    assert str(e.value) == "the f16x2 eval arithmetic is built for FNO3d at width 64 with modes3 <= 16"
    with pytest.raises(NotImplementedError) as e:
        m.set_storage("bf16")
    assert str(e.value) == "bf16 activation storage is built for FNO3d at width 64 with modes3 <= 16"
    assert m.arith == "f32" and len(m._ws) == 2                    # a refusal changes nothing
    m.width = 64
    assert m.set_arith("f16x2") is m and m.arith == "f16x2" and m._ws == {(1, True): "train"}      # the eval workspaces went
