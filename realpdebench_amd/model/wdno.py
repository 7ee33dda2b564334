"""WDNO, the wavelet-domain diffusion operator, on MI355X -- drop-in for ``realpdebench.model.wdno.WDNO`` as ``load_model`` builds it
(reference realpdebench/model/wdno.py, realpdebench/model/load_model.py:24-45): same constructor, ``forward(input[B,T,H,W,C_in]) ->
[B,T_out,H,W,C_out]``, ``train_loss`` as a value, the reference's ``state_dict`` key set (``model.*`` plus the schedule buffers; the
rescaler is a file next to the dataset, as in the reference).  Evaluation only (``_common.EvalByDefault``): a backward raises.

What the model is.  Input and target are taken through one level of a separable 3-D wavelet filter bank (``bior1.1``: 2 taps, ``bior1.3``:
6 taps, zero-padded boundaries); the eight sub-bands of every channel -- a target with ``T_out = r T_in`` enters as ``C_out r`` channels
-- are the channels of a *state* on the coefficient mesh, padded up to the U-Net's stride and divided by a per-column rescaler.  A
Gaussian diffusion (DDIM when ``sampling_timesteps < timesteps``, else the ancestral loop) denoises the target columns while the input
columns and the pad cells are re-imposed after every step; the inverse transform of the target columns is the prediction.

The denoiser is ``realpdebench_amd.model.unet.Unet3d`` with ``in_time = out_time = Tp``: the reference's ``wdno_libs/unet.py`` is its
``unet.py`` without frame replication, and ``WDNO`` calls ``self.model(x, t)`` so that ``t`` lands in the unused ``cond`` argument -- the
network is never told the diffusion step (its time MLP sees zeros).  Its 7x7x7 ``init_conv`` has 8 (C_in + C_out r) input channels here
and runs as the implicit GEMM ``rpb_conv7x`` (``Unet3d.init_conv_implicit``).

Kernel map (C ABI, ``include/rpb.h``): ``rpb_wdno_dec`` (decomposition into state columns; its maximum mode serves ``find_rescaler``),
``rpb_wdno_rec`` (reconstruction, crop and the ``sub_f`` un-permute), ``rpb_wdno_step`` (the whole point-wise part of a sampling step,
both conditions included; the step's scalars are read from a device table built once, so the sampling loop never synchronises with
the host).  Noise comes from one overridable ``sample_noise(shape, device)``, by default ``torch.randn`` on the device in the reference's
call order and shapes, the doubled initial draw of wdno.py:382-383 included.

``ptwt`` / ``pywt`` are not dependencies: the transform's published definition (``ptwt.wavedec3`` / ``waverec3`` with ``mode="zero"``,
``level=1``) is restated in the kernels, and the two filter tables below are the published ``pywt`` constants.

``set_arith("f16x2")`` forwards to the denoiser (its 3x3x3 convolutions); ``rpb_conv7x`` stays on the default arithmetic.
Not built: the training step, ``interpolate``, more than one rank."""
import math
import os

import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

from .. import ops
from ._common import EvalByDefault
from .model import Model

# pywt.Wavelet(name).dec_lo / dec_hi / rec_lo / rec_hi as published
_S = 0.7071067811865476
_Q = 0.08838834764831845
WAVELETS = {
    "bior1.1": ((_S, _S), (-_S, _S), (_S, _S), (_S, -_S)),
    "bior1.3": ((-_Q, _Q, _S, _S, _Q, -_Q), (0.0, 0.0, -_S, _S, 0.0, 0.0), (0.0, 0.0, _S, _S, 0.0, 0.0), (-_Q, -_Q, _S, -_S, _Q, _Q)),
}

SCHEDULE_BUFFERS = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                    "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
                    "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")


def coef_len(n, L):
    """coefficients per axis of one level with zero padding: (2L - 3) // 2 zeros per side, one more for an odd length, stride 2"""
    return (n + L - 1) // 2


def linear_beta_schedule(timesteps):
    scale = 1000 / timesteps
    return torch.linspace(scale * 0.0001, scale * 0.02, timesteps, dtype=torch.float64)


def cosine_beta_schedule(timesteps, s=0.008):
    t = torch.linspace(0, timesteps, timesteps + 1, dtype=torch.float64) / timesteps
    ac = torch.cos((t + s) / (1 + s) * math.pi * 0.5) ** 2
    ac = ac / ac[0]
    return torch.clip(1 - (ac[1:] / ac[:-1]), 0, 0.999)


def sigmoid_beta_schedule(timesteps, start=-3, end=3, tau=1, clamp_min=1e-5):
    t = torch.linspace(0, timesteps, timesteps + 1, dtype=torch.float64) / timesteps
    v_start = torch.tensor(start / tau).sigmoid()
    v_end = torch.tensor(end / tau).sigmoid()
    ac = (-((t * (end - start) + start) / tau).sigmoid() + v_end) / (v_end - v_start)
    ac = ac / ac[0]
    return torch.clip(1 - (ac[1:] / ac[:-1]), 0, 0.999)


BETA_SCHEDULES = {"linear": linear_beta_schedule, "cosine": cosine_beta_schedule, "sigmoid": sigmoid_beta_schedule}


def schedule_buffers(betas):
    """The reference's buffers (wdno.py:202-247) from fp64 ``betas``: name -> fp64 tensor, in registration order."""
    alphas = 1.0 - betas
    ac = torch.cumprod(alphas, dim=0)
    ac_prev = F.pad(ac[:-1], (1, 0), value=1.0)
    pv = betas * (1.0 - ac_prev) / (1.0 - ac)
    return {
        "betas": betas, "alphas_cumprod": ac, "alphas_cumprod_prev": ac_prev,
        "sqrt_alphas_cumprod": torch.sqrt(ac), "sqrt_one_minus_alphas_cumprod": torch.sqrt(1.0 - ac),
        "log_one_minus_alphas_cumprod": torch.log(1.0 - ac), "sqrt_recip_alphas_cumprod": torch.sqrt(1.0 / ac),
        "sqrt_recipm1_alphas_cumprod": torch.sqrt(1.0 / ac - 1), "posterior_variance": pv,
        "posterior_log_variance_clipped": torch.log(pv.clamp(min=1e-20)),
        "posterior_mean_coef1": betas * torch.sqrt(ac_prev) / (1.0 - ac),
        "posterior_mean_coef2": (1.0 - ac_prev) * torch.sqrt(alphas) / (1.0 - ac),
    }


def ddim_time_pairs(total_timesteps, sampling_timesteps):
    """wdno.py:377-380: [(T-1, ...), ..., (t, -1)]"""
    times = torch.linspace(-1, total_timesteps - 1, steps=sampling_timesteps + 1)
    times = list(reversed(times.int().tolist()))
    return list(zip(times[:-1], times[1:]))


def ddim_table(buf, pairs, eta):
    """[steps][5] fp32 = (sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t], sqrt(abar_next), c, sigma) per step, from the
    fp32 buffers in fp32 with the operation order of wdno.py:407-411; the last step (time_next < 0) only uses the first two."""
    rows = []
    for time, time_next in pairs:
        a, b = buf["sqrt_recip_alphas_cumprod"][time], buf["sqrt_recipm1_alphas_cumprod"][time]
        if time_next < 0:
            rows.append(torch.stack([a, b, torch.ones(()), torch.zeros(()), torch.zeros(())]))
            continue
        alpha, alpha_next = buf["alphas_cumprod"][time], buf["alphas_cumprod"][time_next]
        sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
        c = (1 - alpha_next - sigma ** 2).sqrt()
        rows.append(torch.stack([a, b, alpha_next.sqrt(), c, sigma]).float())
    return torch.stack(rows).float().contiguous()


def ancestral_table(buf):
    """[timesteps][5] fp32 = (sqrt_recip, sqrt_recipm1, posterior_mean_coef1, posterior_mean_coef2, exp(0.5 posterior_log_variance_clipped))
    (wdno.py:274-281, 320)."""
    return torch.stack([buf["sqrt_recip_alphas_cumprod"], buf["sqrt_recipm1_alphas_cumprod"], buf["posterior_mean_coef1"],
                        buf["posterior_mean_coef2"], (0.5 * buf["posterior_log_variance_clipped"]).exp()], dim=1).float().contiguous()


def rescaler_path(dataset_root, dataset_name, wave_type, pad_mode):
    return os.path.join(dataset_root, dataset_name, f"wdno_rescaler_{wave_type}_{pad_mode}.pt")


def find_rescaler(train_dataset, wave_type, pad_mode, dataset_root, dataset_name, device, batch_size=64):
    """wdno.py:76-111: the per-column maximum of |coefficient| over ``train_dataset`` (zeros replaced by one), saved next to the dataset
    under the reference's file name and loaded from there when it exists; returned times 1.4 on ``device``."""
    save_path = rescaler_path(dataset_root, dataset_name, wave_type, pad_mode)
    if not os.path.exists(save_path):
        assert train_dataset.dataset_type == "numerical", "Rescaler should be computed on numerical data"
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"{save_path} does not exist and computing it runs on MI355X only: there is no CPU fallback (build the "
                               "model on 'cuda', or provide the file)")
        filt = torch.tensor(WAVELETS[wave_type], dtype=torch.float32, device=device).contiguous()
        L, rows = filt.shape[1], ops.wdno_dec_rows()
        rescaler = None
        for inputs, targets in DataLoader(train_dataset, batch_size=batch_size, shuffle=False, num_workers=0):
            inputs, targets = inputs.to(device).float().contiguous(), targets.to(device).float().contiguous()
            b, f, h, w, c_in = inputs.shape
            r, c_t = targets.shape[1] // f, targets.shape[-1]
            pi = torch.empty(rows, 8 * c_in, device=device)
            pt = torch.empty(rows, 8 * c_t * r, device=device)
            ops.wdno_dec_max(inputs, filt, pi, b, f, h, w, c_in, 1, L)
            ops.wdno_dec_max(targets, filt, pt, b, f, h, w, c_t, r, L)
            m = torch.cat((pi.amax(dim=0), pt.amax(dim=0)))
            rescaler = m if rescaler is None else torch.max(rescaler, m)
        rescaler[rescaler == 0] = 1
        rescaler = rescaler.reshape(1, 1, 1, 1, -1)
        torch.save(rescaler.cpu(), save_path)
    else:
        rescaler = torch.load(save_path)
    return (rescaler * 1.4).to(device)


class WDNO(EvalByDefault, Model):
    batch_independent = True
    training_unavailable = EvalByDefault.TRAIN_MSG.format("WDNO", "WDNO")
    DP_MSG = "WDNO has no training step: data-parallel training is not built"

    def __init__(self, model, train_dataset, dataset_root, dataset_name, wave_type="bior1.3", pad_mode="zero", loss_type="l2",
                 timesteps=1000, beta_schedule="sigmoid", schedule_fn_kwargs=dict(), sampling_timesteps=None, ddim_sampling_eta=0.0):
        super().__init__()
        if wave_type not in WAVELETS:
            raise NotImplementedError(f"WDNO on MI355X: wave_type {wave_type!r} is not built (the configs use {', '.join(WAVELETS)})")
        if pad_mode != "zero":
            raise NotImplementedError(f"WDNO on MI355X: pad_mode {pad_mode!r} is not built (every config uses 'zero')")
        if loss_type not in ("l1", "l2"):
            raise ValueError(f"invalid loss type {loss_type}")
        self.model = model
        self.model.init_conv_implicit = True
        self.channels = self.model.channels
        input, target = train_dataset[0]
        self.input_shape, self.output_shape = tuple(input.shape), tuple(target.shape)
        self.image_size, self.frames = self.input_shape[1], self.input_shape[0]
        T, H, W, c_in = self.input_shape
        if self.output_shape[1:3] != (H, W) or self.output_shape[0] % T:
            raise ValueError(f"WDNO: target {self.output_shape} must share H, W with the input {self.input_shape} and have T_out = r T_in")
        self.sub_frames = self.output_shape[0] // T
        c_out = self.output_shape[-1] * self.sub_frames
        if self.channels != 8 * (c_in + c_out):
            raise ValueError(f"WDNO: the denoiser has {self.channels} channels, the data needs 8 * ({c_in} + {c_out})")
        self.wave_type, self.pad_mode = wave_type, pad_mode
        self.filter_len = len(WAVELETS[wave_type][0])
        self.coef_shape = tuple(coef_len(n, self.filter_len) for n in (T, H, W))
        device = self.model.p("time_mlp.1.weight").device
        self.rescaler = find_rescaler(train_dataset, wave_type, pad_mode, dataset_root, dataset_name, device)
        if self.rescaler.numel() != self.channels:
            raise ValueError(f"WDNO: the rescaler has {self.rescaler.numel()} columns, the state {self.channels}")
        pad_factor = 2 ** len(self.model.in_out)                  # wdno.py:186, 2 ** len(downs)
        self.padded_shape = tuple(((d + pad_factor - 1) // pad_factor) * pad_factor for d in self.coef_shape)
        self.pad_x = self.padded_shape[1] - self.coef_shape[1]
        self.pad_t = self.padded_shape[0] - self.coef_shape[0]
        if self.coef_shape[2] + self.pad_x != self.padded_shape[2]:
            # wdno.py:341 pads W by the pad taken from H: the reference's state then has another W than its noise and fails
            raise ValueError(f"WDNO: coefficient mesh {self.coef_shape} needs pad {self.pad_x} on H but "
                             f"{self.padded_shape[2] - self.coef_shape[2]} on W; the reference applies H's pad to both (wdno.py:341) and "
                             "cannot run this shape")
        if beta_schedule not in BETA_SCHEDULES:
            raise ValueError(f"unknown beta schedule {beta_schedule}")
        betas = BETA_SCHEDULES[beta_schedule](timesteps, **schedule_fn_kwargs)
        self.num_timesteps = int(betas.shape[0])
        self.loss_type = loss_type
        self.sampling_timesteps = sampling_timesteps if sampling_timesteps is not None else self.num_timesteps
        assert self.sampling_timesteps <= self.num_timesteps
        self.is_ddim_sampling = self.sampling_timesteps < self.num_timesteps
        self.ddim_sampling_eta = ddim_sampling_eta
        for name, val in schedule_buffers(betas).items():
            self.register_buffer(name, val.to(torch.float32))
        self._dev = {}                                            # device -> (filters, DDIM table, ancestral table)

    # ------------------------------------------------------------------ device-side constants
    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.rescaler = fn(self.rescaler)
        self._dev = {}
        return out

    def load_state_dict(self, *args, **kwargs):
        self._dev = {}
        return super().load_state_dict(*args, **kwargs)

    def _constants(self, device):
        """(filters [4][L], DDIM table, ancestral table) on ``device``, built once: the sampling loop reads its scalars from there."""
        key = str(device)
        if key not in self._dev:
            buf = {n: getattr(self, n).detach().cpu() for n in SCHEDULE_BUFFERS}
            pairs = ddim_time_pairs(self.num_timesteps, self.sampling_timesteps)
            self._dev[key] = (torch.tensor(WAVELETS[self.wave_type], dtype=torch.float32, device=device).contiguous(),
                              ddim_table(buf, pairs, self.ddim_sampling_eta).to(device), ancestral_table(buf).to(device), pairs)
        return self._dev[key]

    def set_arith(self, arith):
        """Forwards to the denoiser: ``"f16x2"`` moves its 3x3x3 convolutions as it does for ``unet``; ``rpb_conv7x`` and the wavelet and
        step kernels stay on the default arithmetic."""
        super().set_arith(arith)
        self.model.set_arith(arith)
        return self

    def sample_noise(self, shape, device):
        return torch.randn(shape, device=device)

    def check_input(self, shape):
        if tuple(shape[1:]) != self.input_shape or len(shape) != 5:
            raise ValueError(f"WDNO was built for inputs [B, {', '.join(str(s) for s in self.input_shape)}], got {tuple(shape)}")

    # ------------------------------------------------------------------ transform
    def _decompose(self, x, dst, ld, col0, r, filt):
        B = x.shape[0]
        T, H, W, _ = self.input_shape
        ops.wdno_dec(x, filt, self.rescaler.view(-1), dst, B, T, H, W, x.shape[-1], r, self.filter_len, self.padded_shape, ld, col0)

    def _condition(self, input, filt):
        """[B, Tp, Hp, Wp, 8 C_in]: the input's coefficient columns over the rescaler, zero on the pad cells"""
        c8 = 8 * self.input_shape[-1]
        cond = torch.empty(input.shape[0], *self.padded_shape, c8, device=input.device)
        self._decompose(input, cond, c8, 0, 1, filt)
        return cond

    def _reconstruct(self, img, filt):
        B = img.shape[0]
        T, H, W, c_in = self.input_shape
        out = torch.empty(B, *self.output_shape, device=img.device)
        ops.wdno_rec(img, filt, self.rescaler.view(-1), out, B, T, H, W, self.output_shape[-1], self.sub_frames, self.filter_len,
                     self.padded_shape, self.channels, 8 * c_in)
        return out

    def _step(self, mode, B, out, **kw):
        ops.wdno_step(mode, out, B, self.padded_shape, self.coef_shape, self.channels, 8 * self.input_shape[-1], **kw)

    # ------------------------------------------------------------------ sampling
    def _forward_eval(self, input, keep=None):
        """wdno.py:434-438.  ``keep``: a dict that receives the conditioning state and ``img`` after every step (tests)."""
        return (self.ddim_sample if self.is_ddim_sampling else self.p_sample_loop)(input, keep)

    def ddim_sample(self, input, keep=None):
        B, device = input.shape[0], input.device
        filt, table, _, pairs = self._constants(device)
        shape = (B, *self.padded_shape, self.channels)
        img = self.sample_noise(shape, device)
        img = self.sample_noise(shape, device)                     # wdno.py:382-383 draws twice
        cond = self._condition(input, filt)
        self._step(ops.WDNO_START, B, img, noise=img, cond=cond)
        if keep is not None:
            keep["cond"], keep["img"] = cond, []
        for i, (time, time_next) in enumerate(pairs):
            eps = self.model(img).contiguous()
            if time_next < 0:
                self._step(ops.WDNO_DDIM_LAST, B, img, img=img, eps=eps, cond=cond, sc=table[i])
            else:
                noise = self.sample_noise(shape, device)
                self._step(ops.WDNO_DDIM, B, img, img=img, eps=eps, cond=cond, noise=noise, sc=table[i])
            if keep is not None:
                keep["img"].append(img.clone())
        return self._reconstruct(img, filt)

    def p_sample_loop(self, input, keep=None):
        B, device = input.shape[0], input.device
        filt, _, table, _ = self._constants(device)
        shape = (B, *self.padded_shape, self.channels)
        x = self.sample_noise(shape, device)
        cond = self._condition(input, filt)
        self._step(ops.WDNO_START, B, x, noise=x, cond=cond)
        if keep is not None:
            keep["cond"], keep["img"] = cond, []
        for t in reversed(range(self.num_timesteps)):
            eps = self.model(x).contiguous()
            noise = self.sample_noise(shape, device) if t > 0 else None
            self._step(ops.WDNO_ANCESTRAL, B, x, img=x, eps=eps, cond=cond, noise=noise, sc=table[t])
            if keep is not None:
                keep["img"].append(x.clone())
        return self._reconstruct(x, filt)

    def interpolate(self, *args, **kwargs):
        raise NotImplementedError("WDNO.interpolate is not built on MI355X (no evaluation loop of the reference calls it)")

    # ------------------------------------------------------------------ loss as a value
    def train_loss(self, input, target, noise=None, t=None):
        """wdno.py:488-524: the element-wise loss between the denoiser's output on the noised, conditioned state and the conditioned
        noise, as a value (under grad mode it raises).  ``t`` [B] and ``noise`` (state-shaped) default to the reference's draws, in its
        order."""
        if torch.is_grad_enabled():
            raise NotImplementedError(type(self).training_unavailable)
        self.check_input(tuple(input.shape))
        if tuple(target.shape[1:]) != self.output_shape:
            raise ValueError(f"WDNO was built for targets [B, {', '.join(str(s) for s in self.output_shape)}], got {tuple(target.shape)}")
        self._require_hip(input)
        input, target = input.contiguous().float(), target.contiguous().float()
        B, device = input.shape[0], input.device
        filt = self._constants(device)[0]
        if t is None:
            t = torch.randint(0, self.num_timesteps, (B,), device=device).long()
        c8 = 8 * self.input_shape[-1]
        start = torch.empty(B, *self.padded_shape, self.channels, device=device)
        self._decompose(input, start, self.channels, 0, 1, filt)
        self._decompose(target, start, self.channels, c8, self.sub_frames, filt)
        if noise is None:
            noise = self.sample_noise(tuple(start.shape), device)
        sc = torch.stack((self.sqrt_alphas_cumprod[t], self.sqrt_one_minus_alphas_cumprod[t]), dim=1).contiguous()
        state, goal = torch.empty_like(start), torch.empty_like(start)
        self._step(ops.WDNO_QSAMPLE, B, state, img=start, noise=noise.contiguous().float(), sc=sc, out2=goal)
        out = self.model(state)
        return (out - goal) ** 2 if self.loss_type == "l2" else (out - goal).abs()
