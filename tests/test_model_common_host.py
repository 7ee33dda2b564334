"""Host side of realpdebench_amd/model/_common.py (no GPU needed): the invalidation rule of ``LayoutCache``, the stale-layout case it
closes in Transolver._conv_cat (``p.data = other`` leaves ``p._version`` unchanged), and ``HipFunction`` on a pure-torch
model."""
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
