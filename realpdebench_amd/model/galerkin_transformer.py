"""Galerkin Transformer (3-D) on MI355X -- drop-in for ``realpdebench.model.galerkin_transformer.GalerkinTransformer3d``
(reference realpdebench/model/galerkin_transformer.py:11-206), built by ``load_model`` like
``realpdebench/model/load_model.py:77-91`` for the model family every reference YAML selects
(``configs/*/galerkin_transformer.yaml``): galerkin attention, one encoder layer without layer_norm, per-head
LayerNorm on K and V, ``pos=None``, no down/up-scaler, ``ifft2`` decoder with one spectral layer and ``spacial_fc``.

Pipeline (tokens channels-last ``[B*n][256]``, n = T*H*W):
  downscaler Linear (rpb_tokens_lift) -> ONE Q|K|V GEMM (N = 768) -> per-head LayerNorm of K, V (rpb_headnorm) ->
  per (sample, head) ``K^T V / n`` (rpb_head_scores, fp64-reduced chunk partials) -> ``x + drop(Q P)`` with the 64x64
  head matrices in LDS and the residual / dropout fused (rpb_head_apply) -> FeedForward: two token GEMMs (ReLU, dropout,
  residual fused) -> SpectralRegressor: token GEMM + grid/bias/pad scatter, then the FNO3d kernels K2-K7 (truncated DFT
  GEMM stages, mode contraction, 1x1 conv + BatchNorm statistics, crop + Linear + SiLU + Linear).
The encoder's training backward mirrors it with the same kernels (dgrad = token GEMM on the transposed weight, wgrad =
TN GEMM); there is no PyTorch fallback.

``linear_attention`` applies ``F.dropout(p_attn)`` with the functional defaults p=0.5, training=True whatever the
module mode (layers.py:730-731).  Here: training mode draws that p=0.5 mask; eval mode uses the deterministic
expectation (no mask) unless ``eval_attn_dropout=True`` is set on the model.
"""
import math
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import ops
from ._common import HipFunction, wgrad
from .fno import FNO3d
from .model import Model as _ModelBase

_DK = 64          # head width the HIP kernels are built for (n_hidden 256 / n_head 4 in every reference YAML)


class _Lin(nn.Module):
    def __init__(self, fin, fout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(fout, fin))
        self.bias = nn.Parameter(torch.empty(fout))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))          # nn.Linear defaults
        bound = 1.0 / math.sqrt(fin)
        nn.init.uniform_(self.bias, -bound, bound)


class _LN(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))


class _Id(nn.Module):
    """layers.py:21-40: the 'Identity' down-scaler is an nn.Linear named ``id``."""

    def __init__(self, fin, fout):
        super().__init__()
        self.id = _Lin(fin, fout)


class _Attn(nn.Module):
    def __init__(self, d_model, n_head, pos_dim, xavier_init, diagonal_weight, symmetric_init):
        super().__init__()
        self.linears = nn.ModuleList([_Lin(d_model, d_model) for _ in range(3)])
        for lin in self.linears:                                       # layers.py:901-913
            if xavier_init > 0:
                nn.init.xavier_uniform_(lin.weight, gain=xavier_init)
                if diagonal_weight > 0:
                    lin.weight.data += diagonal_weight * torch.eye(d_model)
                if symmetric_init:
                    lin.weight.data += lin.weight.data.T.clone()
                nn.init.constant_(lin.bias, 0)
        self.norm_K = nn.ModuleList([_LN(d_model // n_head) for _ in range(n_head)])
        self.norm_V = nn.ModuleList([_LN(d_model // n_head) for _ in range(n_head)])
        if pos_dim > 0:
            self.fc = _Lin(d_model + n_head * pos_dim, d_model)       # layers.py:825-826: allocated, unused with pos=None


class _FF(nn.Module):
    def __init__(self, d, hid):
        super().__init__()
        self.lr1, self.lr2 = _Lin(d, hid), _Lin(hid, d)


class _Encoder(nn.Module):
    def __init__(self, d_model, n_head, ff, pos_dim, xavier_init, diagonal_weight, symmetric_init):
        super().__init__()
        self.attn = _Attn(d_model, n_head, pos_dim, xavier_init, diagonal_weight, symmetric_init)
        self.ff = _FF(d_model, ff)


class _RegressorCore(FNO3d):
    """``SpectralRegressor`` (galerkin_transformer_libs/model.py:521-638) with one spectral layer IS one FNO3d block of
    width ``freq_dim`` between a Linear(n_hidden+3 -> freq_dim) and a Linear-SiLU-Linear head, so it reuses FNO3d's
    arena, workspace and forward / backward pipelines; only the lift differs: its input is the 256-wide token tensor,
    hence a token GEMM plus the grid / bias / zero-pad scatter instead of the small-C_in lift kernel."""
    proj_act = 1           # SiLU, model.py:631-632
    _lift_wz = None        # the fc weight's fp16 planes while an "f16x2" eval forward of the owning model runs its "fc" site on them

    def _wsplit(self):
        Ch = self.dim_in
        w = self.pview("fc0.weight")
        return w[:, :Ch].contiguous(), w[:, Ch:].contiguous()

    def _alloc_lift_ws(self, ws, f):
        d, C = ws.d, self.width
        ws.gU = torch.empty(d.ncrop, C, **f)
        ws.gx = torch.empty(d.ncrop, self.dim_in, **f)
        ws.lift_rows = ops._lib.query("rpb_lift_bwd_rows")
        ws.lift_part = torch.empty(ws.lift_rows * (C * 3 + C), **f)
        ws.d0 = ops.Dims(d.B, d.T, d.H, d.W, 0, C, self.padding)

    def _lift_fwd(self, x, ws):
        """model.py:612-618: ws.A0 = pad(fc(cat(x, grid))).  x: tokens [B*n][n_hidden]."""
        grids, _ = self._consts(x.device)
        d, C, Ch = ws.d, self.width, self.dim_in
        if not hasattr(ws, "U"):
            ws.U = torch.empty(d.ncrop, C, device=x.device, dtype=torch.float32)
        Wx, Wg = self._wsplit()
        if self._lift_wz is not None:                                  # GalerkinTransformer3d.set_arith("f16x2"), eval forward only
            ops.gemm_nt_f16x2(x, self._lift_wz, ws.U, d.ncrop, C, Ch)
        else:
            ops.gemm_nt(x, Wx, ws.U, d.ncrop, C, Ch)
        ops.pad_grid_fwd(ws.U, grids, Wg, self.pview("fc0.bias"), ws.A0, d)

    def _lift_bwd(self, g, x, ws, gflat):
        """g = dLoss/d(ws.A0): gradients of fc and, in ws.gx, of the encoder output tokens."""
        grids, _ = self._consts(x.device)
        d, C, Ch = ws.d, self.width, self.dim_in
        Wx, _ = self._wsplit()
        ops.crop_gather(g, ws.gU, d)
        ops.lift_bwd(g, ws.gU, grids, ws.lift_part, ws.d0)            # C_in = 0: only the grid columns and the bias
        partl = ws.lift_part.view(ws.lift_rows, C * 3 + C)
        gw = self.pview("fc0.weight", gflat)
        dWg = torch.empty(C, 3, device=g.device, dtype=torch.float32)
        self._reduce_cols(partl, 0, C * 3, dWg)
        self._reduce_cols(partl, C * 3, C, self.pview("fc0.bias", gflat))
        dWx, _ = wgrad(ws.gU, x, d.ncrop, C, Ch, one_reduction=True)
        gw[:, :Ch].copy_(dWx)
        gw[:, Ch:].copy_(dWg)
        ops.gemm_nt(ws.gU, Wx.t().contiguous(), ws.gx, d.ncrop, Ch, C)


_REG_RENAME = (("regressor.fc0.", "regressor.fc."), ("regressor.spectral_convs.", "regressor.spectral_conv."),
               ("regressor.fc1.", "regressor.regressor1."), ("regressor.fc2.", "regressor.regressor2."))


class GalerkinTransformer3d(_ModelBase):
    """``set_arith`` selects the arithmetic of the evaluation / rollout forward's dense token GEMMs: ``"f32"`` (default, the parity path:
    operands as three bf16 planes, six products per fp32 product) or ``"f16x2"`` (opt-in: operands as two fp16 planes, three products,
    dropped term <= 2^-22; one power-of-two scale per weight and one per token row, formed inside the launch; csrc/rpb_gemm3h.hip,
    DESIGN.md section 13.3).  ``F16X2_SITES`` names the GEMMs that move: Q|K|V and FeedForward lr1, the two the kernel is faster on; lr2
    and the regressor's fc are wired but measured slower and stay on the default kernel.  Only the forward without saved activations
    (eval mode under ``torch.no_grad()``) changes; a product whose shape ``rpb_gemm3h_supported`` refuses stays on the default
    kernel, and so does every other kernel of the model.  The training step is the same under either setting."""
    # The token GEMMs set_arith("f16x2") can move to rpb_gemm3h.  Measured at M = 2.6 M rows (profiles/galerkin_arith_probe.txt,
    # DESIGN.md section 13.3): Q|K|V 6.36 -> 5.11 ms and lr1 2.06 -> 1.95 ms are faster; lr2 (residual epilogue, 2.31 -> 4.70 ms) and
    # fc (N = 128, 1.34 -> 1.69 ms) are not and stay on the default kernel.
    ALL_F16X2_SITES = ("qkv", "lr1", "lr2", "fc")
    F16X2_SITES = ("qkv", "lr1")
    F16X2_GEMM = ("gemm3h_supported", "gemm_nt_f16x2")

    def __init__(self, **kwargs):
        super().__init__()
        cfg = dict(kwargs)
        g = cfg.get
        self.n_hidden, self.n_head = int(g("n_hidden", 256)), int(g("n_head", 4))
        unsupported = []
        if g("attention_type", "galerkin") != "galerkin":
            unsupported.append(f"attention_type={g('attention_type')!r}")
        if int(g("num_encoder_layers", 1)) != 1 or g("decoder_type", "ifft2") != "ifft2":
            unsupported.append("num_encoder_layers != 1 or decoder_type != 'ifft2'")
        if int(g("num_regressor_layers", 1)) != 1 or not g("spacial_fc", True) or int(g("spacial_dim", 3)) != 3:
            unsupported.append("num_regressor_layers != 1 / spacial_fc False / spacial_dim != 3")
        if g("layer_norm", False) or not g("attn_norm", True) or g("batch_norm", False) or g("return_attn_weight", False):
            unsupported.append("layer_norm / attn_norm / batch_norm / return_attn_weight differ from the reference YAMLs")
        if g("downscaler_size") or g("upscaler_size") or g("return_latent", False):
            unsupported.append("down/up-scaler or return_latent")
        if g("regressor_activation", "silu") not in (None, "silu"):
            unsupported.append(f"regressor_activation={g('regressor_activation')!r}")
        if self.n_hidden != 4 * _DK or self.n_head != 4:
            unsupported.append(f"n_hidden={self.n_hidden}, n_head={self.n_head} (kernels: 4 heads x 64)")
        if unsupported:
            raise NotImplementedError("MI355X GalerkinTransformer3d covers the configuration family of the reference's "
                                      "configs/*/galerkin_transformer.yaml; unsupported: " + "; ".join(unsupported))
        self.shape_in = tuple(int(v) for v in cfg["shape_in"])
        self.shape_out = tuple(int(v) for v in cfg["shape_out"])
        self.node_feats, self.n_targets = int(cfg["node_feats"]), int(cfg["n_targets"])
        self.dim_ff = int(g("dim_feedforward") or 2 * self.n_hidden)
        if self.dim_ff % 32 or self.node_feats + 3 > 24:
            # node_feats: the down-scaler Linear is rpb_tokens_lift (K <= 32) and its weight gradient rpb_lift_bwd (node_feats + 3
            # <= 24 feature columns; 16 = configs/combustion/galerkin_transformer.yaml is a specialised instance)
            raise NotImplementedError("dim_feedforward must be a multiple of 32 and node_feats <= 21")
        self.norm_eps = float(g("norm_eps") or 1e-5)
        drop = g("encoder_dropout")
        self.p_enc = 0.05 if drop is None else float(drop)             # model.py:47, default(dropout, 0.05)
        fd = g("ffn_dropout")
        self.p_ffn = self.p_enc if fd is None else float(fd)
        self.eval_attn_dropout = False
        C = self.n_hidden
        self.downscaler = _Id(self.node_feats, C)
        self.encoder_layers = nn.ModuleList([_Encoder(C, self.n_head, self.dim_ff, int(g("pos_dim", 1)),
                                                      float(g("xavier_init", 1e-2)), float(g("diagonal_weight", 1e-2)),
                                                      bool(g("symmetric_init", False)))])
        freq = int(g("freq_dim", 128))
        T, H, W = self.shape_in[:3]
        self.regressor = _RegressorCore(int(g("fourier_modes_t", 4)), int(g("fourier_modes_x", 4)),
                                        int(g("fourier_modes_y", 4)), 1, freq, (T, H, W, C), self.shape_out)
        self._mask_override = None      # tests: dict(attn=[B,4,64,64], d1=[M,C], ffn=[M,ff], d2=[M,C]), already scaled
        self.__name__ = "GalerkinTransformer3D"

    # ------------------------------------------------------------------ reference-compatible state dict
    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        sd = OrderedDict() if destination is None else destination
        for name, p in self.named_parameters():
            if not name.startswith("regressor."):
                sd[prefix + name] = p if keep_vars else p.detach().clone()
        for k, v in self.regressor.state_dict(prefix="regressor.").items():
            for a, b in _REG_RENAME:
                if k.startswith(a):
                    k = b + k[len(a):]
                    break
            sd[prefix + k] = v
        return sd

    def load_state_dict(self, state_dict, strict=True, assign=False):
        own = {n: p for n, p in self.named_parameters() if not n.startswith("regressor.")}
        reg = {}
        for k, v in state_dict.items():
            if k.startswith("regressor."):
                for a, b in _REG_RENAME:
                    if k.startswith(b):
                        k = a + k[len(b):]
                        break
                reg[k[len("regressor."):]] = v
        expected = set(self.state_dict().keys())
        missing, unexpected = sorted(expected - set(state_dict)), sorted(set(state_dict) - expected)
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for GalerkinTransformer3d: missing {missing}, "
                               f"unexpected {unexpected}")
        with torch.no_grad():
            for n, p in own.items():
                if n in state_dict:
                    src = torch.as_tensor(state_dict[n])
                    if src.shape != p.shape:
                        raise RuntimeError(f"size mismatch for {n}: {tuple(src.shape)} vs {tuple(p.shape)}")
                    p.copy_(src)
        self.regressor.load_state_dict(reg, strict=False)
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def grads_as_state_dict(self, grads):
        """{parameter: gradient} from ``_backward_hip`` -> {reference parameter name: gradient}."""
        out = OrderedDict()
        for n, p in self.named_parameters():
            if n.startswith("regressor.") or grads.get(p) is None:
                continue
            out[n] = grads[p]
        for k, v in self.regressor.grads_as_state_dict(grads[self.regressor.flat]).items():
            k = "regressor." + k
            for a, b in _REG_RENAME:
                if k.startswith(a):
                    k = b + k[len(a):]
                    break
            out[k] = v
        return out

    # ------------------------------------------------------------------ forward
    def _masks(self, B, M, f):
        """Inverted-dropout multipliers of this step (None = no dropout on that site)."""
        if self._mask_override is not None:
            return dict(self._mask_override)
        mk = {}
        if self.training or self.eval_attn_dropout:                             # layers.py:730-731 (functional defaults)
            mk["attn"] = torch.empty(B, self.n_head, _DK, _DK, **f).bernoulli_(0.5).mul_(2.0)
        if self.training:
            # the three token-sized nn.Dropouts never exist as tensors: each site is a (seed, keep) pair, the mask is
            # generated in the producing kernel's epilogue (Philox keyed on the element index) and regenerated in backward
            seeds = torch.randint(0, 2 ** 62, (3,)).tolist()                    # host RNG: no device sync
            if self.p_enc > 0:
                mk["d1"], mk["d2"] = (seeds[0], 1.0 - self.p_enc), (seeds[1], 1.0 - self.p_enc)
            if self.p_ffn > 0:
                mk["ffn"] = (seeds[2], 1.0 - self.p_ffn)
        return mk

    @staticmethod
    def _site(mk, key):
        """A dropout site of this step -> (mask tensor | None, (seed, keep) | None)."""
        v = mk.get(key)
        if v is None:
            return None, None
        return (None, v) if isinstance(v, tuple) else (v, None)

    @staticmethod
    def _through_dropout(g, site, n):
        """g * mask of a dropout site (backward through nn.Dropout); returns g itself when the site is off."""
        m, d = site
        if m is None and d is None:
            return g
        out = torch.empty_like(g)
        if d is not None:
            ops.dropout_mul(g, out, n, d[0], d[1])
        else:
            ops.mul(g, m, out, n)
        return out

    def _head_products(self, G, ldg, A, lda, B, n, mask):
        """[B,4,64,64] = (G_h^T A_h) / n (x the attention-dropout mask): layers.py:723-731 and its backward."""
        chunks = ops.head_scores_chunks(B, n)
        L = B * self.n_head * _DK * _DK
        part = torch.empty(chunks, L, device=self.regressor.flat.device, dtype=torch.float32)
        ops.head_scores(G, ldg, A, lda, part, B, n)
        S = torch.empty(B, self.n_head, _DK, _DK, device=part.device, dtype=torch.float32)
        ops.reduce_partials(part, chunks, L, out_f32=S.view(-1), scale=1.0 / n)
        if mask is not None:
            S.mul_(mask)                       # 64x64 numbers per head: plumbing-scale torch glue
        return S

    @torch.no_grad()
    def _forward_hip(self, x, save=None):
        B = x.shape[0]
        C, Cin, Fh = self.n_hidden, self.node_feats, self.dim_ff
        n = x[0].numel() // Cin
        M = B * n
        f = dict(device=x.device, dtype=torch.float32)
        new = lambda *shape: torch.empty(*shape, **f)
        enc, at = self.encoder_layers[0], self.encoder_layers[0].attn
        mk = self._masks(B, M, f)
        x2 = x.reshape(M, Cin)
        X0 = new(M, C)
        ops.tokens_lift(x2, self.downscaler.id.weight.data, self.downscaler.id.bias.data, X0, M, Cin, C, False)
        # ---- attention (layers.py:829-899): fused Q|K|V projection, per-head LayerNorm of K and V
        ran = [] if self.arith == "f16x2" and save is None else None      # the f16x2 eval forward: the sites it moved
        QKV = new(M, 3 * C)
        cat_b = lambda: torch.cat([l.bias.data for l in at.linears], 0)
        # (the f16x2 eval forward caches the concatenated bias like the weight's planes: a routed Q|K|V forms no concatenation per call)
        bqkv = cat_b() if ran is None else self._layouts.get("f16x2_qkv_bias", [l.bias for l in at.linears], cat_b)
        Wqkv = self._dense(ran, "qkv", "qkv", [l.weight for l in at.linears], lambda: torch.cat([l.weight.data for l in at.linears], 0),
                           X0, QKV, M, 3 * C, C, bias=bqkv)
        gK, bK = torch.cat([m.weight.data for m in at.norm_K]), torch.cat([m.bias.data for m in at.norm_K])
        gV, bV = torch.cat([m.weight.data for m in at.norm_V]), torch.cat([m.bias.data for m in at.norm_V])
        KVn = new(M, 2 * C)
        ops.headnorm_fwd(QKV, 3 * C, gK, bK, KVn, 2 * C, M, C, self.norm_eps, col0=C, ocol0=0)
        ops.headnorm_fwd(QKV, 3 * C, gV, bV, KVn, 2 * C, M, C, self.norm_eps, col0=2 * C, ocol0=C)
        # ---- p_attn = drop(K^T V / n) per sample and head (layers.py:723-731), x1 = x0 + drop(Q p_attn) (model.py:112-116)
        P = self._head_products(ops.Sub(KVn, 0), 2 * C, ops.Sub(KVn, C), 2 * C, B, n, mk.get("attn"))
        X1 = new(M, C)
        m1, dr1 = self._site(mk, "d1")
        ops.head_apply(ops.Sub(QKV, 0), 3 * C, P, X1, C, B, n, residual=X0, ldr=C, mask=m1, ldm=C, drop=dr1)
        # ---- x2 = x1 + drop(lr2(drop(relu(lr1(x1)))))  (layers.py:979-987, model.py:120-121)
        Hh = new(M, Fh)
        mf, drf = self._site(mk, "ffn")
        lr1, lr2 = enc.ff.lr1, enc.ff.lr2                               # (a dropout site set through _mask_override keeps its kernel)
        self._dense(ran, "lr1", "lr1", [lr1.weight], lr1.weight.data, X1, Hh, M, Fh, C, bias=lr1.bias.data, act=3, mask=mf, drop=drf)
        X2 = new(M, C)
        m2, dr2 = self._site(mk, "d2")
        self._dense(ran, "lr2", "lr2", [lr2.weight], lr2.weight.data, Hh, X2, M, C, Fh, bias=lr2.bias.data, residual=X1, mask=m2, drop=dr2)
        # ---- spectral regressor (model.py:600-638)
        reg = self.regressor
        training = save is not None
        ws = reg._workspace(B, training, x.device)
        # FNO3d._forward_impl is the pipeline every FNO3d subclass and the trainers share and it calls _lift_fwd(x, ws) with that fixed
        # signature, so the fc planes travel as an attribute of the regressor for the duration of this call only (cleared on any exit)
        reg._lift_wz = self._routed_planes(ran, "fc", "fc", [reg.flat], lambda: reg._wsplit()[0], M, reg.width, C)
        try:
            out = reg._forward_impl(X2, ws, training=training)
            if reg._lift_wz is not None:
                ran.append("fc")
        finally:
            reg._lift_wz = None
        if ran is not None:
            self.f16x2_ran = tuple(s for s in self.ALL_F16X2_SITES if s in ran)
        if save is not None:
            save.update(x2=x2, X0=X0, QKV=QKV, KVn=KVn, P=P, X1=X1, Hh=Hh, X2=X2, mk=mk, ws=ws, B=B, n=n, M=M,
                        Wqkv=Wqkv, gK=gK, gV=gV)
        return reg._shape_output(out.clone(), B)

    # ------------------------------------------------------------------ backward
    @torch.no_grad()
    def _backward_hip(self, sv, g_out, need_gx=False):
        """Gradients of every parameter given dLoss/d(out): autograd of galerkin_transformer.py:20-63."""
        C, Fh, Cin = self.n_hidden, self.dim_ff, self.node_feats
        B, n, M, mk = sv["B"], sv["n"], sv["M"], sv["mk"]
        f = dict(device=g_out.device, dtype=torch.float32)
        new = lambda *shape: torch.empty(*shape, **f)
        T_ = lambda w: w.data.t().contiguous()
        enc, at, reg, ws = self.encoder_layers[0], self.encoder_layers[0].attn, self.regressor, sv["ws"]
        grads = {}
        gflat = torch.zeros_like(reg.flat)
        reg._backward_impl(sv["X2"], reg._unshape_grad(g_out, B), ws, gflat)
        grads[reg.flat] = gflat
        early = getattr(self, "_dp_early", None)
        if early is not None:              # data parallel: the 99 % of the gradient bytes that are final already start their RCCL
            early(reg.flat, gflat)         # all-reduce on the side stream and overlap the encoder's backward below
        g = ws.gx                                                     # dLoss/dX2
        # ---- FeedForward
        g2 = self._through_dropout(g, self._site(mk, "d2"), M * C)
        grads[enc.ff.lr2.weight], grads[enc.ff.lr2.bias] = wgrad(g2, sv["Hh"], M, C, Fh, one_reduction=True)
        gH = new(M, Fh)
        mf, drf = self._site(mk, "ffn")
        ops.gemm_nt(g2, T_(enc.ff.lr2.weight), gH, M, Fh, C, act=4, aux=sv["Hh"], mask=mf, drop=drf)
        grads[enc.ff.lr1.weight], grads[enc.ff.lr1.bias] = wgrad(gH, sv["X1"], M, Fh, C, one_reduction=True)
        gX1 = new(M, C)
        ops.gemm_nt(gH, T_(enc.ff.lr1.weight), gX1, M, C, Fh, residual=g)
        del gH
        # ---- attention output: x1 = x0 + d1 * (Q P)
        ga = self._through_dropout(gX1, self._site(mk, "d1"), M * C)
        QKV, KVn, P = sv["QKV"], sv["KVn"], sv["P"]
        dS = self._head_products(ops.Sub(QKV, 0), 3 * C, ga, C, B, n, mk.get("attn"))      # dL/d(K^T V), masked, / n
        gQKV, gKVn = new(M, 3 * C), new(M, 2 * C)
        tr = lambda w: w.transpose(-1, -2).contiguous()
        ops.head_apply(ga, C, tr(P), ops.Sub(gQKV, 0), 3 * C, B, n)                                  # dQ  = g P^T
        ops.head_apply(ops.Sub(KVn, C), 2 * C, tr(dS), ops.Sub(gKVn, 0), 2 * C, B, n)               # dKn = Vn dS^T
        ops.head_apply(ops.Sub(KVn, 0), 2 * C, dS, ops.Sub(gKVn, C), 2 * C, B, n)                   # dVn = Kn dS
        rows = ops.headnorm_bwd_rows(M)
        hp = new(rows, 2 * C)
        for which, norms, gam in ((0, at.norm_K, sv["gK"]), (1, at.norm_V, sv["gV"])):
            ops.headnorm_bwd(QKV, 3 * C, gam, gKVn, 2 * C, gQKV, 3 * C, hp, M, C, self.norm_eps,
                             col0=(1 + which) * C, gcol0=which * C, xcol0=(1 + which) * C)
            dgb = new(2 * C)
            ops.reduce_partials(hp, rows, 2 * C, out_f32=dgb)
            for h, m in enumerate(norms):
                grads[m.weight] = dgb[h * _DK:(h + 1) * _DK].clone()
                grads[m.bias] = dgb[C + h * _DK:C + (h + 1) * _DK].clone()
        del gKVn
        dW, db = wgrad(gQKV, sv["X0"], M, 3 * C, C, one_reduction=True)
        for i, lin in enumerate(at.linears):
            grads[lin.weight], grads[lin.bias] = dW[i * C:(i + 1) * C].clone(), db[i * C:(i + 1) * C].clone()
        gX0 = new(M, C)
        ops.gemm_nt(gQKV, sv["Wqkv"].t().contiguous(), gX0, M, C, 3 * C, residual=gX1)
        del gQKV
        # ---- down-scaler Linear(node_feats -> n_hidden): skinny weight gradient = the FNO lift-backward reduction on the
        #      unpadded token layout (pad 0); its three grid columns are not parameters here and are dropped
        T, H, W = self.shape_in[:3]
        grids, _ = reg._consts(g_out.device)
        d_tok = ops.Dims(B, T, H, W, Cin, C, 0)
        rows = ops._lib.query("rpb_lift_bwd_rows")
        lp = new(rows, C * (Cin + 3) + C)
        ops.lift_bwd(gX0, sv["x2"], grids, lp, d_tok)
        dWf, db = new(C, Cin + 3), new(C)
        ops.reduce_partials(lp, rows, C * (Cin + 3), out_f32=dWf.view(-1), row_stride=lp.shape[1])
        ops.reduce_partials(lp, rows, C, out_f32=db, row_stride=lp.shape[1], col0=C * (Cin + 3))
        grads[self.downscaler.id.weight], grads[self.downscaler.id.bias] = dWf[:, :Cin].contiguous(), db
        return grads

    # ------------------------------------------------------------------ Model protocol
    def forward(self, node, pos=None, grid=None, weight=None, boundary_value=None):
        if pos is not None or grid is not None or weight is not None:
            raise NotImplementedError("pos / grid / weight inputs are never used by the reference's train/eval loops")
        self._require_hip(node)
        if tuple(node.shape[1:]) != self.shape_in:
            raise ValueError(f"expected input [B,{','.join(map(str, self.shape_in))}], got {tuple(node.shape)}")
        x = node.contiguous().float()
        params = list(self.parameters())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            if not self.training:
                raise NotImplementedError("gradients through eval-mode BatchNorm are not implemented; wrap evaluation in "
                                          "torch.no_grad() as the reference does (train.py:345-361)")
            return HipFunction.apply(x, self, *params)
        return self._forward_hip(x, save={} if self.training else None)
