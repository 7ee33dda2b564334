"""TEST INFRASTRUCTURE ONLY -- a plain-torch restatement of WDNO (realpdebench/model/wdno.py) in any dtype, shared by
tests/golden/make_golden_wdno.py, tests/test_wdno_host.py and the GPU tests (a plain helper module: no conftest, no fixture).

``ptwt`` / ``pywt`` are third-party packages that are not installed here; what the reference calls from them is restated from their
published definitions:

* ``Wavelet``: the filter tables of ``pywt.Wavelet("bior1.1")`` / ``("bior1.3")``;
* ``wavedec3(data, wavelet, mode="zero", level=1)``: per axis ``(2L - 3) // 2`` zeros on each side, one more on the right of an odd
  length, then a stride-2 ``conv3d`` (a cross-correlation) with the outer products of the REVERSED decomposition filters; the result is
  ``[aaa, {"aad": ..., "ada": ..., "add": ..., "daa": ..., "dad": ..., "dda": ..., "ddd": ...}]``, first letter = first (T) axis;
* ``waverec3(coefs, wavelet)``: stride-2 ``conv_transpose3d`` with the outer products of the reconstruction filters, then
  ``(2L - 3) // 2`` samples trimmed per side.

The vectors of tests/golden/wdno_small.npz were made with these functions standing in for the packages, so they pin everything AROUND
the transform; the transform itself is pinned by properties (tests/test_wdno_host.py): perfect reconstruction at even and odd lengths,
and known answers on unit impulses.

The rest restates the model: state columns (``dec_state`` / ``rec_state``), one sampling step per mode (``step``), the schedule, and the
two samplers and the loss around a denoiser given as a callable."""
import contextlib

import torch
import torch.nn.functional as F

_S, _Q = 0.7071067811865476, 0.08838834764831845
TABLES = {
    "bior1.1": dict(dec_lo=[_S, _S], dec_hi=[-_S, _S], rec_lo=[_S, _S], rec_hi=[_S, -_S]),
    "bior1.3": dict(dec_lo=[-_Q, _Q, _S, _S, _Q, -_Q], dec_hi=[0.0, 0.0, -_S, _S, 0.0, 0.0], rec_lo=[0.0, 0.0, _S, _S, 0.0, 0.0],
                    rec_hi=[-_Q, -_Q, _S, -_S, _Q, _Q]),
}
SUBBANDS = ("aaa", "aad", "ada", "add", "daa", "dad", "dda", "ddd")
DDIM, DDIM_LAST, ANCESTRAL, QSAMPLE, START = range(5)


class Wavelet:
    """stands where ``pywt.Wavelet(name)`` stands in the reference"""

    def __init__(self, name):
        self.name = name
        for k, v in TABLES[name].items():
            setattr(self, k, list(v))
        self.dec_len = self.rec_len = len(self.dec_lo)


def coef_len(n, L):
    return (n + L - 1) // 2


def _filters3(lo, hi, like):
    lo, hi = torch.tensor(lo, dtype=like.dtype, device=like.device), torch.tensor(hi, dtype=like.dtype, device=like.device)
    f = {"a": lo, "d": hi}
    return torch.stack([torch.einsum("i,j,k->ijk", f[s[0]], f[s[1]], f[s[2]]) for s in SUBBANDS]).unsqueeze(1)     # [8,1,L,L,L]


def wavedec3(data, wavelet, mode="zero", level=1):
    """data [N, T, H, W] -> [aaa, {aad..ddd}] each [N, Tc, Hc, Wc]"""
    assert mode == "zero" and level == 1
    L = len(wavelet.dec_lo)
    p = (2 * L - 3) // 2
    pad = []
    for n in reversed(data.shape[-3:]):                    # F.pad takes the last axis first
        pad += [p, p + n % 2]
    x = F.pad(data.unsqueeze(1), pad)
    res = F.conv3d(x, _filters3(wavelet.dec_lo[::-1], wavelet.dec_hi[::-1], data), stride=2)
    return [res[:, 0], {s: res[:, i] for i, s in enumerate(SUBBANDS) if i}]


def waverec3(coefs, wavelet):
    """the inverse of one level: [aaa, {aad..ddd}] -> [N, 2 Tc + L - 2 - 2 p, ...]"""
    L = len(wavelet.rec_lo)
    p = (2 * L - 3) // 2
    x = torch.stack([coefs[0]] + [coefs[1][s] for s in SUBBANDS[1:]], dim=1)
    y = F.conv_transpose3d(x, _filters3(wavelet.rec_lo, wavelet.rec_hi, x), stride=2)[:, 0]
    if p:
        y = y[:, p:-p, p:-p, p:-p]
    return y


# ---------------------------------------------------------------------------------- state columns
def virtual_channels(x, r):
    """x [B, r T, H, W, C] -> [B, T, H, W, C r], channel c r + sub = frame sub T + t of channel c (wdno.py:493-495)"""
    B, TT, H, W, C = x.shape
    return x.reshape(B, r, TT // r, H, W, C).permute(0, 2, 3, 4, 5, 1).reshape(B, TT // r, H, W, C * r)


def dec_state(x, r, wave, rescaler, padded):
    """x [B, r T, H, W, C] -> [B, Tp, Hp, Wp, 8 C r]: column 8 cv + s = sub-band s of virtual channel cv over rescaler[column], zero on
    the pad cells.  ``rescaler`` None: the bare coefficients."""
    v = virtual_channels(x, r)
    B, T, H, W, Cv = v.shape
    c = wavedec3(v.permute(0, 4, 1, 2, 3).reshape(B * Cv, T, H, W), Wavelet(wave))
    t = torch.stack([c[0]] + [c[1][s] for s in SUBBANDS[1:]], dim=1)                       # [B Cv, 8, Tc, Hc, Wc]
    Tc, Hc, Wc = t.shape[-3:]
    t = t.reshape(B, Cv * 8, Tc, Hc, Wc)
    t = F.pad(t, (0, padded[2] - Wc, 0, padded[1] - Hc, 0, padded[0] - Tc)).permute(0, 2, 3, 4, 1)
    return t if rescaler is None else t / rescaler.to(t.dtype)


def rec_state(cols, wave, rescaler, shape, C, r):
    """cols [B, Tp, Hp, Wp, 8 C r] -> [B, r T, H, W, C] (wdno.py:422-430 for the output columns)"""
    T, H, W = shape
    L = len(TABLES[wave]["dec_lo"])
    Tc, Hc, Wc = (coef_len(n, L) for n in shape)
    B = cols.shape[0]
    t = (cols * rescaler.to(cols.dtype)).permute(0, 4, 1, 2, 3)[:, :, :Tc, :Hc, :Wc].reshape(B * C * r, 8, Tc, Hc, Wc)
    y = waverec3([t[:, 0], {s: t[:, i] for i, s in enumerate(SUBBANDS) if i}], Wavelet(wave))
    y = y.reshape(B, C * r, *y.shape[1:])[:, :, :T, :H, :W]
    return y.reshape(B, C, r, T, H, W).permute(0, 2, 3, 4, 5, 1).reshape(B, r * T, H, W, C)


def conditions(state, cond, coef):
    """set_input_condition + set_pad_condition (wdno.py:476-486), on a copy"""
    state = state.clone()
    if cond is not None:
        state[..., :cond.shape[-1]] = cond
    state[:, coef[0]:] = 0
    state[:, :, coef[1]:] = 0
    state[:, :, :, coef[2]:] = 0
    return state


def step(mode, coef, img=None, eps=None, cond=None, noise=None, sc=None):
    """one call of rpb_wdno_step: ``sc`` five scalars (QSAMPLE: [B][2]); returns out (QSAMPLE: (out, target))"""
    if mode == START:
        return conditions(noise, cond, coef)
    if mode == QSAMPLE:
        sa, sb = (sc[:, k].reshape(-1, 1, 1, 1, 1) for k in (0, 1))
        n_in = cond.shape[-1]
        return (conditions(sa * img + sb * noise, img[..., :n_in], coef), conditions(noise, torch.zeros_like(img[..., :n_in]), coef))
    x0 = (sc[0] * img - sc[1] * eps).clamp(-1.0, 1.0)
    if mode == DDIM_LAST:
        out = x0
    elif mode == DDIM:
        e2 = (sc[0] * img - x0) / sc[1]
        out = x0 * sc[2] + sc[3] * e2 + sc[4] * noise
    else:
        out = sc[2] * x0 + sc[3] * img
        if noise is not None:
            out = out + sc[4] * noise
    return conditions(out, cond, coef)


# ---------------------------------------------------------------------------------- the model around a denoiser
@contextlib.contextmanager
def default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


class Plan:
    """Shapes of one WDNO instance, from the rule of wdno.py:179-191 without a sample transform."""

    def __init__(self, shape_in, shape_out, wave, n_res):
        self.shape_in, self.shape_out, self.wave = tuple(shape_in), tuple(shape_out), wave
        self.L = len(TABLES[wave]["dec_lo"])
        self.r = shape_out[0] // shape_in[0]
        self.c_in, self.c_out = shape_in[-1], shape_out[-1]
        self.channels = 8 * (self.c_in + self.c_out * self.r)
        self.coef = tuple(coef_len(n, self.L) for n in shape_in[:3])
        f = 2 ** n_res
        self.padded = tuple((d + f - 1) // f * f for d in self.coef)


def ddim_pairs(total, steps):
    times = list(reversed(torch.linspace(-1, total - 1, steps=steps + 1).int().tolist()))
    return list(zip(times[:-1], times[1:]))


def ddim_scalars(buf, pairs, eta):
    """[steps][5] in the dtype of ``buf`` (the registered buffers, cast): what wdno.py:249-253, 407-411 compute per step.  The reference's
    fp64 run forms them in fp64 from its fp32-rounded buffers; its fp32 run in fp32."""
    rows = []
    for time, nxt in pairs:
        a, b = buf["sqrt_recip_alphas_cumprod"][time], buf["sqrt_recipm1_alphas_cumprod"][time]
        if nxt < 0:
            rows.append(torch.stack([a, b, torch.ones_like(a), torch.zeros_like(a), torch.zeros_like(a)]))
            continue
        alpha, alpha_next = buf["alphas_cumprod"][time], buf["alphas_cumprod"][nxt]
        sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
        rows.append(torch.stack([a, b, alpha_next.sqrt(), (1 - alpha_next - sigma ** 2).sqrt(), sigma]))
    return torch.stack(rows)


def ancestral_scalars(buf):
    return torch.stack([buf["sqrt_recip_alphas_cumprod"], buf["sqrt_recipm1_alphas_cumprod"], buf["posterior_mean_coef1"],
                        buf["posterior_mean_coef2"], (0.5 * buf["posterior_log_variance_clipped"]).exp()], dim=1)


def start_state(plan, input, target, rescaler):
    cols = [dec_state(input, 1, plan.wave, None, plan.padded)]
    if target is not None:
        cols.append(dec_state(target, plan.r, plan.wave, None, plan.padded))
    t = torch.cat(cols, dim=-1)
    return t / rescaler.reshape(-1)[:t.shape[-1]].to(t.dtype)


def ddim_sample(unet, plan, tables, input, rescaler, noises):
    """wdno.py:368-432.  ``tables``: [steps][5] (the model's ``ddim_table``); ``noises``: the start state's noise, then one per step but
    the last.  Returns (cond, [img after every step], output)."""
    dt = input.dtype
    cond = start_state(plan, input, None, rescaler)
    noises = [n.to(dt) for n in noises]
    img = step(START, plan.coef, noise=noises[0], cond=cond)
    imgs = []
    for i in range(tables.shape[0]):
        eps = unet(img)
        last = i == tables.shape[0] - 1
        img = step(DDIM_LAST if last else DDIM, plan.coef, img=img, eps=eps, cond=cond, noise=None if last else noises[1 + i],
                   sc=tables[i].to(dt))
        imgs.append(img)
    out = rec_state(img[..., 8 * plan.c_in:], plan.wave, rescaler.reshape(-1)[8 * plan.c_in:], plan.shape_in[:3], plan.c_out, plan.r)
    return cond, imgs, out


def ancestral_sample(unet, plan, table, input, rescaler, noises):
    """wdno.py:325-366.  ``table``: [timesteps][5] (``ancestral_table``); ``noises``: start, then one per step with t > 0."""
    dt = input.dtype
    cond = start_state(plan, input, None, rescaler)
    noises = [n.to(dt) for n in noises]
    x = step(START, plan.coef, noise=noises[0], cond=cond)
    imgs, k = [], 1
    for t in reversed(range(table.shape[0])):
        eps = unet(x)
        x = step(ANCESTRAL, plan.coef, img=x, eps=eps, cond=cond, noise=noises[k] if t > 0 else None, sc=table[t].to(dt))
        k += 1
        imgs.append(x)
    out = rec_state(x[..., 8 * plan.c_in:], plan.wave, rescaler.reshape(-1)[8 * plan.c_in:], plan.shape_in[:3], plan.c_out, plan.r)
    return cond, imgs, out


def train_loss(unet, plan, sa, sb, input, target, rescaler, noise, t):
    """wdno.py:488-524 with l2: ``sa`` / ``sb`` = sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod"""
    dt = input.dtype
    start = start_state(plan, input, target, rescaler)
    sc = torch.stack((sa[t], sb[t]), dim=1).to(dt)
    state, goal = step(QSAMPLE, plan.coef, img=start, noise=noise.to(dt), cond=start[..., :8 * plan.c_in], sc=sc)
    return (unet(state) - goal) ** 2


def rescaler_of(plan, inputs, targets):
    """find_rescaler's maximum (wdno.py:83-105) over a dataset given as two stacked tensors, before the x 1.4: [1,1,1,1,channels]"""
    m = start_state(plan, inputs, targets, torch.ones(plan.channels))[:, :plan.coef[0], :plan.coef[1], :plan.coef[2]]
    m = m.abs().reshape(-1, plan.channels).amax(dim=0)
    m[m == 0] = 1
    return m.reshape(1, 1, 1, 1, -1)
