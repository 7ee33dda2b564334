"""Plumbing the models share between their parameter trees and the C ABI: the autograd glue (``HipFunction``), the weight-gradient
finish (``wgrad``, ``colsum``, ``sum_rows``), the weight matrices of a padded 3x3x3 convolution and of its data gradient (``padded_weight``,
``flipped_weight``, ``weight_grad_view``), batch-statistics BatchNorm on rows (``batch_norm_rows``, ``batch_norm_rows_bwd``), the cache of
kernel-side layouts (``LayoutCache``) and the base of the models that evaluate by default and train by opt-in (``EvalByDefault``: MWT3d,
DeepONet, CNO3d)."""
import torch

from .. import ops

# checkpoint key -> meta-data key handed back to the caller (train.py:299-301 uses the returned dict)
META_KEYS = {
    "train_losses": "all_train_losses",
    "val_losses": "all_val_losses",
    "iteration": "iteration",
    "best_iteration": "best_iteration",
    "best_val_loss": "best_val_loss",
}


class HipFunction(torch.autograd.Function):
    """Autograd glue of every ``nn.Parameter`` model: one forward / backward call into its HIP pipelines.

    The model provides ``_new_state()`` (what the forward records into: a dict, U-Net's tape), ``_forward_hip(x, state)`` and
    ``_backward_hip(state, g_out, need_gx=...) -> {parameter: gradient}``, with the input gradient under ``"__x__"`` where the model
    computes one (DPOT's sliding windows)."""

    @staticmethod
    def forward(ctx, x, model, *params):
        state = model._new_state()
        out = model._forward_hip(x, state)
        ctx.model, ctx.state, ctx.params = model, state, params
        return out

    @staticmethod
    def backward(ctx, g_out):
        grads = ctx.model._backward_hip(ctx.state, g_out.contiguous().float(), need_gx=ctx.needs_input_grad[0])
        ctx.state = None               # the saved activations go now, not when autograd drops the graph
        return (grads.get("__x__"), None) + tuple(grads.get(p) for p in ctx.params)


def wgrad(G, A, M, N, K, ldg=None, lda=None, conv=None, conv_mode=1, one_reduction=False):
    """(dW [N,K], db [N]) = (G^T A(im2col), colsum G): TN GEMM (``ops.conv3_wgrad_parts`` for the 3x3x3 convolution) into split-token
    partials, then the fp64 reduction.  ``one_reduction``: a single launch over ``[dW | db]`` whose results are views of one buffer and
    which may wait for the end of a ``deferred_reductions`` block; otherwise two launches into separate tensors.  The reduction kernel
    is chosen by row length and the two kernels add rows in a different order, so the forms differ in the low bits of ``db``: a call
    site keeps the form it has."""
    dev = (G.t if isinstance(G, ops.Sub) else G).device
    taps_rev = False
    if conv is not None and conv_mode == 1:
        part, taps_rev = ops.conv3_wgrad_parts(G, A, M, N, K // 27, conv, ldg=ldg, ldx=lda)
    else:
        part = torch.empty(ops.gemm_tn_splits(M, N, K, conv is not None, conv_mode, ldg=ldg, lda=lda), N * K + N, device=dev,
                           dtype=torch.float32)
        ops.gemm_tn(G, A, part, M, N, K, ldg=ldg, lda=lda, conv=conv, conv_mode=conv_mode)
    splits, L = part.shape
    if one_reduction:
        tot = torch.empty(L, device=dev, dtype=torch.float32)
        ops.reduce_partials(part, splits, L, out_f32=tot, deferrable=not taps_rev)       # (the tap restore below reads dW at once)
        dW, db = tot[:N * K].view(N, K), tot[N * K:]
    else:
        dW, db = torch.empty(N, K, device=dev, dtype=torch.float32), torch.empty(N, device=dev, dtype=torch.float32)
        ops.reduce_partials(part, splits, N * K, out_f32=dW.view(-1), row_stride=L)
        ops.reduce_partials(part, splits, N, out_f32=db, row_stride=L, col0=N * K)
    if taps_rev:
        dW = ops.conv3_taps_restore(dW, N, K // 27)
    return dW, db


def sum_rows(part, rows, L, f64=False, deferrable=False):
    """sum_r part[r][:L] in fp64, returned as fp32 (or as the fp64 sums themselves)."""
    out = torch.empty(L, device=part.device, dtype=torch.float64 if f64 else torch.float32)
    ops.reduce_partials(part, rows, L, out_f64=out if f64 else None, out_f32=None if f64 else out, deferrable=deferrable)
    return out


def colsum(x, M, N, deferrable=False):
    """Column sums of x [M][N] (bias gradients) in column chunks the reduction kernel takes (a power of two <= 1024)."""
    rows = ops.colsum_rows()
    chunk = 1024
    while N % chunk:
        chunk //= 2
    out = torch.empty(N, device=x.device, dtype=torch.float32)
    for c0 in range(0, N, chunk):
        part = torch.empty(rows, chunk, device=x.device, dtype=torch.float32)      # one per chunk: the reduction may be deferred
        ops.colsum(ops.Sub(x, c0), part, M, chunk, ld=N)
        ops.reduce_partials(part, rows, chunk, out_f32=ops.Sub(out, c0), deferrable=deferrable)
    return out


def padded_weight(conv, N, K):
    """Conv3d weight [Co][Ci][3][3][3] -> [N][27 * K] fp32, tap-major and channel-minor rows, zero rows / columns on the pad channels."""
    w = conv.weight.detach()
    Co, Ci = w.shape[:2]
    wm = torch.zeros(N, 27, K, dtype=torch.float32, device=w.device)
    wm[:Co, :, :Ci] = w.permute(0, 2, 3, 4, 1).reshape(Co, 27, Ci)
    return wm.reshape(N, 27 * K)


def flipped_weight(conv, N, K):
    """Data-gradient weights of a Conv3d(Ci, Co, 3, padding=1): the same convolution run from the Co side with flipped, transposed taps,
    Wd[ci][(kt, kh, kw)][co] = W[co][ci][2 - kt][2 - kh][2 - kw] -> [K][27 * N] fp32 (K >= Ci output rows, N >= Co input channels, zero on
    the pad channels): what ``padded_weight`` is to the forward convolution."""
    w = conv.weight.detach()
    Co, Ci = w.shape[:2]
    wd = torch.zeros(K, 27, N, dtype=torch.float32, device=w.device)
    wd[:Ci, :, :Co] = w.flip(2, 3, 4).permute(1, 2, 3, 4, 0).reshape(Ci, 27, Co)
    return wd.reshape(K, 27 * N)


def weight_grad_view(dW, Co, Ci, N, K):
    """dW [N][27 * K] (tap-major rows, the layout of ``padded_weight``) -> the parameter's [Co][Ci][3][3][3]."""
    return dW.view(N, 3, 3, 3, K)[:Co, :, :, :, :Ci].permute(0, 4, 1, 2, 3).contiguous()


def reduces_stats(sync):
    """Does ``sync`` (None, or ``dp.StatsSync``) sum the BatchNorm statistics over its ranks?  A one-rank group has nothing to sum and runs
    the plain launches, unless ``sync_stats_always`` asks for every launch of the N-rank step (RPB_DP_SYNCBN_ALWAYS=1)."""
    return sync is not None and (sync.world_size > 1 or sync.sync_stats_always)


def batch_norm_rows(y, ld, M, C, bn, parts=None, sync=None):
    """Batch statistics of y [M][ld] (csrc/rpb_rowbn.hip) -> ab [4][C] = (a, b, mean, rstd), a = gamma rstd, b = beta - mean a; the running
    statistics of ``bn`` are updated on the device (``num_batches_tracked`` is the caller's).  C = 256 runs as two column halves.
    ``parts``: fp64 partials already accumulated (a forward in chunks of samples), [2 if C == 256 else 1][rows][2 Ch].
    ``sync`` (``dp.StatsSync``; None: one rank, today's launches): SyncBN over its W ranks, each with M rows (equal per-rank batches, as
    in FNO3d's SyncBN).  The local partials are summed in their fixed order (``rowbn_sum64``), the sums of all halves travel in ONE
    all-reduce, and ``rowbn_finish_sums`` forms the statistics of the M_total = W M rows (biased variance; the running variance with
    M_total / (M_total - 1)): every rank then holds the same ab and the same running statistics.  The call is collective.
    M_total < 2 raises torch's ValueError before anything is launched (CNO3d cannot get there: its input has T > in_dim >= 1, so M >= 2);
    the version counters of the running statistics are bumped here, once per call."""
    reduces = reduces_stats(sync)
    Mt = M * sync.world_size if reduces else M
    if Mt < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size [{Mt} cells, {C} channels]")
    Ch, nh = min(C, 128), max(1, C // 128)
    if parts is None:
        parts = torch.empty(nh, ops.rowbn_rows(), 2 * Ch, device=y.device, dtype=torch.float64)
        for h in range(nh):
            ops.rowbn_stats(ops.Sub(y, h * Ch), ld, M, Ch, parts[h])
    ab = torch.empty(4, C, device=y.device, dtype=torch.float32)
    if reduces:
        sums = torch.empty(nh, 2 * Ch, device=y.device, dtype=torch.float64)
        for h in range(nh):
            ops.rowbn_sum64(parts[h], parts.shape[1], Ch, sums[h])
        sync.all_reduce_sum(sums.view(-1))
    for h in range(nh):
        o = h * Ch
        out = (ops.Sub(bn.weight.data, o), ops.Sub(bn.bias.data, o), ops.Sub(bn.running_mean, o), ops.Sub(bn.running_var, o), bn.eps,
               bn.momentum, *(ops.Sub(ab, k * C + o) for k in range(4)))
        if reduces:
            ops.rowbn_finish_sums(sums[h], Mt, Ch, *out)
        else:
            ops.rowbn_finish(parts[h], parts.shape[1], M, Ch, *out)
    torch.autograd.graph.increment_version(bn.running_mean)           # written through raw pointers: the layout cache is keyed on these
    torch.autograd.graph.increment_version(bn.running_var)
    return ab


def batch_norm_rows_bwd(part, gv, ldg, y, ldy, ab, M, C, Cpad, act, dy, ldd, dy_planes=None, ldp=0, sync=None):
    """The tail of a BatchNorm backward, from the fp64 partials ``part`` [rows][2 C] of (sum dz, sum dz xhat): their fixed-order sum, then
    dy = a (dz - sum dz / M - xhat sum dz xhat / M) as fp32 rows (``dy`` may be ``gv``) and bf16 planes.  Returns (dgamma, dbeta).
    ``sync`` (as in ``batch_norm_rows``; the call is collective): the sums inside dy are those of all W ranks (one all-reduce of a copy)
    over M_total = W M rows, while dgamma and dbeta stay this rank's own sums -- each rank differentiates the mean over ITS samples, and
    the trainer's mean over the ranks turns them into the gradients of the global batch (the global sums there would be W times too
    large)."""
    sums = torch.empty(2 * C, device=part.device, dtype=torch.float64)
    dgb = torch.empty(2, C, device=part.device, dtype=torch.float32)
    ops.rowbn_sum64(part, part.shape[0], C, sums)
    if reduces_stats(sync):
        gsums = sums.clone()
        sync.all_reduce_sum(gsums)
        ops.rowbn_act_bwd_apply_sync(gv, ldg, M, M * sync.world_size, C, Cpad, act, y, ldy, ab[0], ab[1], ab[2], ab[3], sums, gsums, dy=dy,
                                     ldd=ldd, dy_planes=dy_planes, ldp=ldp, dgamma=dgb[0], dbeta=dgb[1])
    else:
        ops.rowbn_act_bwd_apply(gv, ldg, M, C, Cpad, act, y=y, ldy=ldy, a=ab[0], b=ab[1], mean=ab[2], rstd=ab[3], sums=sums, dy=dy, ldd=ldd,
                                dy_planes=dy_planes, ldp=ldp, dgamma=dgb[0], dbeta=dgb[1])
    return dgb[0], dgb[1]


class LayoutCache:
    """Kernel-side layouts derived from parameters and buffers (re-laid-out, concatenated or split weights), one entry per key.

    An entry is served only while every source tensor still has the address, in-place version and device it was built from, the
    caller's ``extra`` key is the same, and ``invalidate()`` has not been called since.  ``_version`` alone is not enough:
    ``p.data = other`` rebinds a parameter without touching it.  The entry therefore holds the (detached) tensors it was built from,
    so that their storage cannot be freed and handed to a new tensor that would stamp the same.  Kernels that write weights through
    raw pointers report it with ``torch.autograd.graph.increment_version`` (``trainer.ArenaTrainer.step``)."""

    def __init__(self):
        self._entries, self._token = {}, 0

    def invalidate(self):
        """``Model`` calls this from ``load_state_dict`` and ``_apply`` (``.to``, ``.float`` ...)."""
        self._token += 1

    def get(self, key, sources, build, extra=None):
        """``build()``'s value for ``key``; ``sources``: the tensors it reads."""
        sources = tuple(sources)
        stamp = (self._token, extra, tuple((t.data_ptr(), t._version, t.device) for t in sources))
        hit = self._entries.get(key)
        if hit is None or hit[0] != stamp:
            hit = self._entries[key] = (stamp, build(), tuple(t.detach() for t in sources))
        return hit[1]


class EvalByDefault:
    """Mixin in front of ``Model`` for MWT3d, DeepONet and CNO3d: evaluation by default, training by opt-in.

    By default an instance covers the evaluation forward, ``train_loss`` as a value, the rollout and checkpoint I/O; every attempt to
    backpropagate raises ``NotImplementedError`` with the class's ``training_unavailable`` instead of returning tensors without a
    graph, and ``trainer.make_trainer`` refuses at construction.  ``enable_training()`` (``hip_training: true`` through ``load_model``)
    opts ONE instance in -- the class and every other instance stay as they are: in ``train()`` mode ``forward`` / ``train_loss`` then
    run through ``HipFunction``, ``eval()`` mode stays the evaluation forward and still refuses a graph.

    A model provides ``training_unavailable`` (``TRAIN_MSG.format(family, class name)``), ``DP_MSG``, ``BATCH_STATISTICS``,
    ``check_input(shape)``, ``_forward_eval(x, ...)`` (runs under ``torch.no_grad()``) and ``_forward_hip`` / ``_backward_hip``."""
    TRAIN_MSG = ("the {} training step is not built yet: {} on MI355X covers the evaluation forward, train_loss as a value under "
                 "torch.no_grad(), the rollout and checkpoint I/O")
    training_unavailable = None        # the class's refusal; None on an enabled instance
    hip_training = False               # enable_training() sets it on the instance
    dp_unavailable = None              # enabled instances: why trainer.make_trainer refuses more than one rank (the class's DP_MSG)
    DP_MSG = None                      # the class's reason
    sync_bn = False                    # enable_training(sync_bn=True) sets it on the instance: BatchNorm over the global batch
    bn_sync = None                     # the ``dp.StatsSync`` a trainer attaches to a ``sync_bn`` instance under a process group
    # The class's training step computes BatchNorm statistics over the batch: they couple the samples of a step, so an enabled instance
    # stops declaring ``batch_independent`` (no micro-batching).
    BATCH_STATISTICS = False

    def enable_training(self, sync_bn=False):
        """Opt this instance into the HIP training step (``hip_training: true`` in a config).

        ``sync_bn`` (``sync_bn: true`` next to it; the ``BATCH_STATISTICS`` models, CNO3d and DeepONet): the instance trains
        data-parallel.  ``trainer.make_trainer`` then accepts more than one rank (``dp_unavailable`` is None) and attaches a
        ``dp.StatsSync`` as ``bn_sync``; BatchNorm statistics and their backward sums are taken over the global batch
        (``batch_norm_rows``), so N ranks with B / N samples each take the step one rank takes on all B samples.  Per-rank batches must
        be equal.  Every ``train()``-mode forward of such an instance under a process group is COLLECTIVE, a ``torch.no_grad()`` one
        included: all ranks must call it together.  ``eval()`` mode uses the running statistics and is untouched.  On one rank the flag
        changes no launch."""
        if sync_bn and not self.BATCH_STATISTICS:
            raise ValueError(f"{type(self).__name__} has no BatchNorm statistics to synchronise: sync_bn is for CNO3d and DeepONet")
        self.hip_training = True
        self.training_unavailable = None
        if self.BATCH_STATISTICS:
            self.batch_independent = False
        self.sync_bn = bool(sync_bn)
        self.dp_unavailable = None if self.sync_bn else self.DP_MSG
        return self

    def _require_eval(self, x):
        """Never hand back a tensor that silently carries no graph.  Under grad mode anything that asks for a gradient is refused
        (inference goes through torch.no_grad(), as rollout.py and eval.py do, or through parameters with requires_grad off).  The
        message is the class's: an enabled instance refuses in ``eval()`` mode with the same words."""
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(type(self).training_unavailable)

    def _require_hip(self, x):
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on MI355X only: there is no CPU fallback (move the model and its input to "
                               "'cuda')")

    def forward(self, x, **eval_args):
        """One order of refusals for every mode: the input's shape, what cannot be differentiated, the device."""
        self.check_input(tuple(x.shape))
        if self.hip_training and self.training:      # the opt-in training step, through HipFunction
            assert not eval_args, eval_args
            if torch.is_grad_enabled() and x.requires_grad:
                raise NotImplementedError(f"{type(self).__name__} training computes no input gradient (no trainer asks for one)")
            self._require_hip(x)
            if not torch.is_grad_enabled():
                return self._forward_hip(x, None)
            return HipFunction.apply(x, self, *self.parameters())
        self._require_eval(x)
        self._require_hip(x)
        with torch.no_grad():
            return self._forward_eval(x.contiguous().float(), **eval_args)

    def train_loss(self, input, target):
        """Elementwise ``mse_loss(pred, target)`` (the reference's): with a graph on an enabled instance in ``train()`` mode, otherwise
        as a value -- under grad mode it raises."""
        if not (self.hip_training and self.training) and torch.is_grad_enabled():
            raise NotImplementedError(type(self).training_unavailable)
        return super().train_loss(input, target)

    def load_checkpoint(self, checkpoint_path, device="cpu"):
        """The base class's loader (``model_state_dict`` + bookkeeping, realpdebench/model/model.py); a bare weights file gives the
        bookkeeping entries of an untrained run (iteration 0, no losses).  (MWT3d matches keys and shapes instead, as its reference does.)"""
        ck = torch.load(checkpoint_path, map_location="cpu")
        if "model_state_dict" in ck:
            meta = super().load_checkpoint(checkpoint_path, "cpu")
        else:
            self.load_state_dict(ck)
            meta = self._bookkeeping({})
        self.to(device)
        return meta

    @staticmethod
    def _bookkeeping(book):
        """The meta data of a checkpoint dict; a bare weights file (``book = {}``) gives the entries of an untrained run."""
        blank = {"train_losses": [], "val_losses": {}, "iteration": 0, "best_iteration": 0, "best_val_loss": float("inf")}
        return {meta: book.get(key, blank[key]) for key, meta in META_KEYS.items()}
