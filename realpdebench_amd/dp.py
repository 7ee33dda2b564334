"""Data parallelism for the FNO3d step: one process per GPU, trajectories sharded across ranks, gradients
summed with RCCL (``torch.distributed`` backend "nccl" on ROCm) over xGMI.

The reference has no distributed path at all (single process, realpdebench/train.py:63); this is new design:

* the flat gradient arena is cut into per-layer buckets that become ready in reverse layer order during the
  backward pass; each bucket's all-reduce is issued asynchronously the moment its last kernel is enqueued, so
  RCCL (running on its own HIP stream) overlaps the remaining backward kernels.  For the cylinder config that is
  4 buckets of 100.7 MB (one ``spectral_convs.{l}`` each, layer 0's still ahead of ~3.5 ms of backward) + 2 small ones;
* BatchNorm3d uses global batch statistics (SyncBN): the fp64 per-channel (sum, sum-of-squares) and the backward
  (sum gz, sum gz*shat) vectors are all-reduced on the compute stream (2*C numbers per layer), so an N-rank step
  equals the 1-rank step on the concatenated batch;
* the loss gradient is pre-scaled by 1/N_global, so the bucket reduction is a plain SUM.

Everything here works on CPU tensors with the gloo backend too (tests/test_dp_gloo.py).
"""
import atexit
import ctypes
import os
import weakref

import torch
import torch.distributed as dist

_LIVE_COMMS = weakref.WeakSet()


def _close_all():
    """Interpreter exit: abort (never a blocking destroy -- a peer may be gone), and only while the process group still exists:
    after ``destroy_process_group`` the ranks no longer shut down together and the communicator is simply left to the OS."""
    for c in list(_LIVE_COMMS):
        try:
            if dist.is_available() and dist.is_initialized():
                c.close(abort=True)
        except Exception:
            pass


atexit.register(_close_all)


class RcclComm:
    """The C-ABI collective (include/rpb.h ``rpb_dp_*``: RCCL all-reduce on a side HIP stream) for CUDA tensors.

    ``torch.distributed`` is only the launcher's rendezvous here: it carries the 128-byte RCCL unique ids from rank 0 to the
    others; the gradient traffic itself goes librpb_hip.so -> librccl.so -> xGMI.

    ONE communicator by default: ``handle`` carries the gradient buckets on the side stream AND the few-hundred-byte SyncBN
    statistics on the compute stream; RCCL orders the operations of one communicator, so a statistics reduction queues behind a
    bucket that is still in flight.  The backward pass announces a layer's 100 MB bucket ~3 ms of kernels before the next
    statistics reduction (model/fno.py: the bucket goes out after ``mode_contract_wgrad``, the reduction after the layer's
    data-gradient ``cell_mix``), so at xGMI rates (100 MB over 8 ranks: < 1 ms) nothing is exposed.  ``RPB_DP_TWO_COMMS=1`` gives
    the statistics their own communicator (``small``): concurrent communicators on two streams are only safe when every rank
    schedules them in the same order, which stream scheduling does not guarantee (round-3 advisor finding) -- it stays opt-in
    until an N > 1 run on hardware has exercised it (tests/test_gpu_rccl_abi.py holds the multi-GPU-gated test)."""

    def __init__(self, process_group=None):
        from . import _lib
        self._lib = _lib
        _lib.load()
        self.rank, self.world_size = dist.get_rank(process_group), dist.get_world_size(process_group)
        self.handle = self._init_comm(process_group)
        two = os.environ.get("RPB_DP_TWO_COMMS") == "1" and os.environ.get("RPB_DP_ONE_COMM") != "1"
        self.small = self._init_comm(process_group) if two else self.handle
        self.closed = False
        _LIVE_COMMS.add(self)

    def _init_comm(self, process_group):
        _lib = self._lib
        buf = (ctypes.c_char * 128)()
        if self.rank == 0:
            _lib.call("rpb_dp_unique_id", ctypes.addressof(buf))
        box = [bytes(buf)]
        dist.broadcast_object_list(box, src=0, group=process_group)
        idbuf = (ctypes.c_char * 128).from_buffer_copy(box[0])
        h = ctypes.c_void_p()
        _lib.call("rpb_dp_allreduce_init", ctypes.addressof(idbuf), self.rank, self.world_size, ctypes.addressof(h))
        return h.value

    @staticmethod
    def _dtype(t):
        if t.dtype == torch.float32:
            return 0
        if t.dtype == torch.float64:
            return 1
        raise TypeError(f"rpb_dp all-reduce: fp32 / fp64 only, got {t.dtype}")

    def _live(self):
        if self.closed:
            raise RuntimeError("rpb_dp: the RCCL communicator of this trainer was closed; build a new DataParallel / trainer")

    def enqueue(self, t):
        """Sum ``t`` (contiguous CUDA tensor / slice) in place across ranks on the side stream, after the work queued so far."""
        self._live()
        assert t.is_cuda and t.is_contiguous()
        self._lib.call("rpb_dp_allreduce_enqueue", self.handle, t.data_ptr(), t.numel(), self._dtype(t),
                       torch.cuda.current_stream().cuda_stream)

    def wait(self):
        self._live()
        self._lib.call("rpb_dp_allreduce_wait", self.handle, torch.cuda.current_stream().cuda_stream)

    def reduce_scatter(self, t):
        """Sum ``t`` over the ranks in place on the side stream; rank r keeps the sum of piece r (``t.numel()`` a multiple of the world size)."""
        self._live()
        assert t.is_cuda and t.is_contiguous()
        self._lib.call("rpb_dp_reduce_scatter_enqueue", self.handle, t.data_ptr(), t.numel(), self._dtype(t),
                       torch.cuda.current_stream().cuda_stream)

    def all_gather(self, t):
        """Every rank's piece of ``t`` reaches all ranks, in place, on the side stream (after the work queued on the current stream)."""
        self._live()
        assert t.is_cuda and t.is_contiguous()
        self._lib.call("rpb_dp_allgather_enqueue", self.handle, t.data_ptr(), t.numel(), self._dtype(t),
                       torch.cuda.current_stream().cuda_stream)

    def mark(self, idx):
        self._live()
        self._lib.call("rpb_dp_mark", self.handle, int(idx))

    def wait_mark(self, idx):
        self._live()
        self._lib.call("rpb_dp_wait_mark", self.handle, int(idx), torch.cuda.current_stream().cuda_stream)

    def set_model(self, world, gbps, lat_us=0.0):
        """One-GPU proxy of an N-rank run: every collective idles its stream for the modelled ring transfer (0 ranks = off)."""
        for h in {self.handle, self.small}:
            self._lib.call("rpb_dp_set_model", h, int(world), float(gbps), float(lat_us))

    def inline(self, t):
        self._live()
        assert t.is_cuda and t.is_contiguous()
        self._lib.call("rpb_dp_allreduce_inline", self.small, t.data_ptr(), t.numel(), self._dtype(t),
                       torch.cuda.current_stream().cuda_stream)

    def close(self, abort=False):
        """Destroy the communicators (trainer teardown; idempotent).  ``abort`` (interpreter exit): ``ncclCommAbort`` instead of
        ``ncclCommDestroy`` -- destroy waits for outstanding collectives and would hang forever when a peer rank has died."""
        if self.handle:
            fn = "rpb_dp_allreduce_abort" if abort else "rpb_dp_allreduce_destroy"
            if self.small and self.small != self.handle:
                self._lib.call(fn, self.small)
            self._lib.call(fn, self.handle)
            self.handle = self.small = None
        self.closed = True
        _LIVE_COMMS.discard(self)

    # ---- instrumentation (bench.py N > 1 line)
    def set_timing(self, on=True):
        for h in {self.handle, self.small}:
            self._lib.call("rpb_dp_set_timing", h, int(on))

    def step_times(self):
        """After ``torch.cuda.synchronize()``: the last step's bucket schedule and the inline (SyncBN) reduction costs."""
        def read(h):
            out = (ctypes.c_float * 1024)()
            n = self._lib.load().rpb_dp_step_times(h, ctypes.addressof(out), 1024)
            if n < 0:
                raise self._lib.RpbError("rpb_dp_step_times failed")
            return list(out[:n])
        b = read(self.handle)
        nb = int(b[0])
        res = {"buckets": [{"start_ms": b[4 + 3 * i], "ms": b[5 + 3 * i], "MB": b[6 + 3 * i] / 1e6} for i in range(nb)],
               "exposed_ms": b[2], "first_announce_to_last_done_ms": b[3]}
        ni_main = int(b[1])
        if len(b) > 4 + 3 * nb + ni_main:       # sharded step: what the forward pass after it waited for parameter gathers (per-bucket marks)
            res["gather_exposed_ms"] = b[4 + 3 * nb + ni_main]
        s = read(self.small)
        ni, off = int(s[1]), 4 + 3 * int(s[0])
        res["inline_ms"] = s[off:off + ni]
        return res


def use_rccl_abi(t=None, process_group=None):
    """The C-ABI RCCL path serves CUDA tensors under the nccl backend of ``process_group`` (default group when None); gloo groups
    (CPU tests, ranks sharing one GPU) and RPB_DP_TORCH=1 keep ``torch.distributed`` collectives."""
    if os.environ.get("RPB_DP_TORCH") == "1" or not dist.is_initialized() or dist.get_backend(process_group) != "nccl":
        return False
    if t is not None and not t.is_cuda:
        return False
    from . import _lib
    if not _lib.query("rpb_dp_available"):        # no loadable librccl.so (the same answer on every rank of a node): ProcessGroupNCCL
        import logging                             # still works, only the side-stream scheduling is torch's instead of ours
        logging.warning("rpb_dp: librccl.so could not be resolved by librpb_hip.so; gradients go through torch.distributed")
        return False
    return True


def layer_buckets(seg, n_layers, total):
    """Contiguous [start, end) ranges of the flat arena in the order the backward pass completes them:
    tail (fc1, fc2), layers L-1 .. 0 (each complete right after its spectral weight gradient), then the small fc0 head,
    so that the last 100 MB bucket still overlaps the tail of the backward pass (layer 0's data gradient + lift)."""
    def start_of(name):
        return seg[name][0]

    cuts = [start_of(f"spec.{l}") for l in range(n_layers)] + [start_of("fc1.weight")]
    buckets = [(cuts[-1], total)]
    for l in range(n_layers - 1, -1, -1):
        buckets.append((cuts[l], cuts[l + 1]))
    buckets.append((0, cuts[0]))
    return buckets


class StatsSync:
    """SyncBN-only hook for models whose parameter gradients are reduced by the trainer after backward (the Galerkin
    Transformer: its spectral regressor is an FNO block with a training-mode BatchNorm3d, galerkin_transformer_libs/
    model.py:572,622): global-batch statistics forward and backward, no gradient buckets.  ``trainer.ArenaTrainer`` also attaches one, as
    ``bn_sync``, to a CNO3d or DeepONet instance enabled with ``sync_bn=True`` (``model._common.batch_norm_rows``).
    ``sync_stats_always`` (RPB_DP_SYNCBN_ALWAYS=1, as for ``DataParallel``): a one-rank group runs the reductions anyway, so that its step
    contains every launch of the N-rank step."""

    def __init__(self, process_group=None, comm=None):
        self.group = process_group
        self.world_size = dist.get_world_size(process_group)
        self.rank = dist.get_rank(process_group)
        self.comm = comm
        self.sync_stats_always = os.environ.get("RPB_DP_SYNCBN_ALWAYS") == "1"

    def all_reduce_sum(self, t):
        if self.comm is not None and t.is_cuda:
            self.comm.inline(t)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)

    def bucket_ready(self, grad, hold_small_of=None):
        pass

    def small_ready(self, grad, l):
        pass


class PeerExchange:
    """Opt-in gradient exchange + optimizer step over PEER POINTERS (``DataParallel(model, p2p=True)`` / RPB_DP_P2P=1; C ABI
    ``rpb_dp_p2p_*``, csrc/rpb_p2p.hip; SURVEY.md section 5.8: direct reduce-scatter + all-gather over the fully connected xGMI mesh
    instead of RCCL's ring).  Every rank exports its gradient arena, its parameter arena and a 256-byte flag block through CUDA IPC
    (``torch.multiprocessing.reductions.reduce_tensor`` -- the same handles ``torch.multiprocessing`` ships tensors with; torch is the
    memory plumbing, ``torch.distributed`` carries the pickled handles once), opens everyone else's, and hands the raw device pointers to
    the library.  Per step: ``adam(...)`` where the all-reduce path calls ``rpb_adam_step`` (rank r sums slice r of all W gradient
    arenas, updates it, stores the new parameters into all W parameter arenas), ``params_wait()`` before the parameters are read again.
    Ranks may share one GPU (the protocol test: RCCL refuses that, peer pointers do not).  No gradient-norm clipping on this path."""

    def __init__(self, flat, grad, process_group=None, timeout_ms=None):
        from torch.multiprocessing.reductions import reduce_tensor
        from . import _lib
        self._lib = _lib
        _lib.load()
        self.group = process_group
        self.rank, self.world = dist.get_rank(process_group), dist.get_world_size(process_group)
        assert flat.is_cuda and grad.is_cuda and flat.is_contiguous() and grad.is_contiguous() and flat.numel() == grad.numel()
        self.flags = torch.zeros(2 * 16, dtype=torch.int64, device=flat.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=flat.device)
        torch.cuda.synchronize(flat.device)
        mine = [reduce_tensor(t) for t in (grad, flat, self.flags)]          # [(rebuild_fn, args)] -- picklable IPC handles
        everyone = [None] * self.world
        dist.all_gather_object(everyone, mine, group=process_group)
        self.views = []                                                       # the opened peer tensors must outlive the handle
        for q in range(self.world):
            self.views.append((grad, flat, self.flags) if q == self.rank else tuple(fn(*args) for fn, args in everyone[q]))
        for g, p, f in self.views:
            assert g.numel() == grad.numel() and p.numel() == flat.numel() and f.numel() == 32, "ranks disagree about the arena"
        arr = lambda i: (ctypes.c_void_p * self.world)(*[v[i].data_ptr() for v in self.views])
        self._arrs = (arr(0), arr(1), arr(2))
        h = ctypes.c_void_p()
        tmo = int(timeout_ms if timeout_ms is not None else os.environ.get("RPB_DP_P2P_TIMEOUT_MS", "20000"))
        _lib.call("rpb_dp_p2p_init", self.rank, self.world, ctypes.addressof(self._arrs[0]), ctypes.addressof(self._arrs[1]),
                  ctypes.addressof(self._arrs[2]), self.status.data_ptr(), flat.numel(), tmo, ctypes.addressof(h))
        self.handle = h.value
        self.step_done = 0            # last step whose PARAM_DONE this rank still has to wait for (0 = none pending)
        dist.barrier(group=process_group)     # nobody writes a flag before everybody has mapped everybody

    def owned(self):
        a, n = ctypes.c_long(), ctypes.c_long()
        self._lib.call("rpb_dp_p2p_slice", self.handle, ctypes.addressof(a), ctypes.addressof(n))
        return a.value, n.value

    def adam(self, m, v, lr, beta1, beta2, eps, step, gscale):
        self._lib.call("rpb_dp_p2p_adam", self.handle, m.data_ptr(), v.data_ptr(), float(lr), float(beta1), float(beta2), float(eps),
                       int(step), float(gscale), torch.cuda.current_stream().cuda_stream, label="dp_p2p_adam")
        self.step_done = int(step)

    def params_wait(self):
        """The current stream waits until every rank has written its slice of THIS rank's parameter arena (and is done reading this
        rank's gradient arena).  No-op when nothing is pending."""
        if self.step_done:
            self._lib.call("rpb_dp_p2p_wait", self.handle, 1, self.step_done, torch.cuda.current_stream().cuda_stream)
            self.step_done = 0

    def check(self):
        """Host check of the status word (one sync): raises if a wait timed out on a silent peer."""
        s = int(self.status.item())
        if s:
            raise RuntimeError(f"rpb_dp_p2p: rank {self.rank} timed out waiting for rank {s - 1} (its process is gone or stalled)")

    def close(self):
        if self.handle:
            torch.cuda.synchronize()
            self._lib.call("rpb_dp_p2p_destroy", self.handle)
            self.handle = None
            self.views = []


class DataParallel:
    """``shard_optimizer`` (or RPB_DP_SHARD_ADAM=1): the optimizer step is sharded over the ranks (ZeRO-1 shape).  Every chunk of a layer's
    spectral gradient whose length divides by 4 * world is REDUCE-SCATTERED instead of all-reduced (rank r owns piece r), Adam runs on the
    owned pieces only (1 / world of the arena: every rank otherwise repeats the same 2.8 GB update, 0.5 ms that no batch size shrinks),
    and the parameter pieces are ALL-GATHERED on the side stream in the order the next forward pass needs them; that pass waits per
    layer (``params_ready``).  The same bytes cross the links as with the all-reduce; the small pieces keep the all-reduce and are
    updated by every rank.  ``shard_world`` > world_size is the one-GPU proxy of bench.py: pieces are sized for that many ranks (the
    rank updates 1 / shard_world of the arena; the step is then no longer a valid training step)."""

    def __init__(self, model, process_group=None, shard_optimizer=None, shard_world=None, p2p=None):
        if not dist.is_initialized():
            raise RuntimeError("torch.distributed must be initialised before DataParallel (one process per GPU)")
        self.model = model
        self.group = process_group
        self.world_size = dist.get_world_size(process_group)
        self.rank = dist.get_rank(process_group)
        self.buckets = layer_buckets(model._seg, model.n_layers, model.flat.numel())
        # a bucket travels as all-reduces of at most chunk_elems elements (16 MB): with ONE communicator RCCL runs operations in issue
        # order, so an inline SyncBN reduction on the compute stream queues behind whatever is in flight -- at most one chunk (~0.1 ms over
        # xGMI) instead of a whole 100 MB bucket (>= 0.5 ms, more than the kernels between two reductions of a B = 4 strong-scaling step)
        self.chunk_elems = max(256, int(float(os.environ.get("RPB_DP_CHUNK_MB", "16")) * (1 << 20) / 4) // 256 * 256)   # (1 KB granules)
        self.shard_opt = bool(shard_optimizer) if shard_optimizer is not None else os.environ.get("RPB_DP_SHARD_ADAM") == "1"
        self.shard_world = int(shard_world or self.world_size)
        if self.shard_world != self.world_size and self.world_size != 1:
            # pieces are cut by shard_world, the collectives by the communicator's size: anything else than the one-rank proxy of bench.py
            # would update the wrong pieces with unreduced gradients
            raise ValueError(f"shard_world={self.shard_world} != world_size={self.world_size}: only a one-rank group may model a larger "
                             "world (bench.py's proxy)")
        if len(self.buckets) > 16:
            raise ValueError(f"{len(self.buckets)} gradient buckets (n_layers + 2): rpb_dp_mark keeps 16 marks per communicator")
        self._step_sharded = False    # this step's big chunks travel as reduce-scatter (only the fused Trainer can consume that)
        # p2p: the fused Trainer exchanges gradients and parameters over peer pointers (PeerExchange) -- no bucket travels at all
        self.p2p_opt = bool(p2p) if p2p is not None else os.environ.get("RPB_DP_P2P") == "1"
        self.peer = None              # PeerExchange, built by the trainer once it has its gradient arena
        self._step_p2p = False
        self._plan = None
        self._pending = False         # sharded step: parameter all-gathers are in flight on the side stream
        self._works = []
        self._next = 0
        self._held = {}
        # one-rank groups skip the SyncBN reductions (nothing to sum); the strong-scaling proxy of bench.py turns them on anyway so
        # that the step it times contains every launch of the N-rank step (RPB_DP_SYNCBN_ALWAYS=1 does the same)
        self.sync_stats_always = os.environ.get("RPB_DP_SYNCBN_ALWAYS") == "1"
        self.comm = RcclComm(process_group) if use_rccl_abi(model.flat, process_group) else None      # C-ABI RCCL on a side stream
        model.dp = self
        self.sync_parameters()

    def sync_parameters(self):
        """Rank 0's weights and BatchNorm buffers become everyone's (the reference has one process: one init)."""
        dist.broadcast(self.model.flat.data, src=0, group=self.group)
        for b in (self.model.bn_running_mean, self.model.bn_running_var, self.model.bn_num_batches_tracked):
            dist.broadcast(b, src=0, group=self.group)

    # ---- small synchronous reductions (SyncBN statistics)
    def all_reduce_sum(self, t):
        self._live()
        if self.comm is not None and t.is_cuda:
            self.comm.inline(t)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)

    # ---- bucketed, overlapped gradient reduction
    def begin_step(self, grad, sharded=False, p2p=False):
        """``sharded``: the caller consumes REDUCE-SCATTERED gradients (the fused ``Trainer.step``: Adam on the owned pieces, then
        ``gather_params``).  Every other caller -- the autograd path (`_FNO3dFunction.backward` + a torch optimizer), a trainer that
        clips by the whole gradient -- gets the plain all-reduce whatever ``shard_opt`` says: a reduce-scattered arena is only
        summed in the piece this rank owns (round-5 advisor finding)."""
        self._live()
        self._works, self._next, self._held = [], 0, {}
        self._step_sharded = bool(sharded) and self.shard_opt
        self._step_p2p = bool(p2p) and self.peer is not None      # the caller reduces inside its optimizer step: nothing to enqueue

    def chunks(self, s, e):
        """[s, e) cut into pieces of at most ``chunk_elems`` elements (the same cut on every rank)."""
        return [(a, min(a + self.chunk_elems, e)) for a in range(s, e, self.chunk_elems)]

    # ---- sharded optimizer step
    def parts(self, bi):
        """The pieces bucket ``bi`` travels in: a layer bucket is its 100 MB spectral range (``big``) and the 17 KB tail from
        ``convs.l.weight`` on (final ~3 ms later in the backward pass, see ``bucket_ready``); the head and tail buckets are one piece."""
        s, e = self.buckets[bi]
        L = self.model.n_layers
        if 1 <= bi <= L:
            cut = self.model._seg[f"convs.{L - bi}.weight"][0]
            if s < cut < e:
                return [(s, cut, True), (cut, e, False)]
        return [(s, e, False)]

    def _sharded(self, a, b, big):
        return self.shard_opt and big and (b - a) % (4 * self.shard_world) == 0

    def shard_plan(self):
        """(pieces, chunks): ``chunks[bi]`` = [(a, b, sharded)] for bucket ``bi``; ``pieces`` = the (start, count) ranges this rank
        updates, in arena order: its piece of every sharded chunk and the whole of every other chunk (identical on all ranks there)."""
        if self._plan is None:
            W, r = self.shard_world, self.rank % self.shard_world
            chunks, pieces = [], []
            for bi in range(len(self.buckets)):
                row = []
                for s0, e0, big in self.parts(bi):
                    for a, b in self.chunks(s0, e0):
                        sh = self._sharded(a, b, big)
                        row.append((a, b, sh))
                        n = (b - a) // W if sh else b - a
                        pieces.append((a + r * n if sh else a, n))
                chunks.append(row)
            pieces.sort()
            self._plan = (pieces, chunks)
        return self._plan

    def owned_table(self, device):
        """Device table for rpb_adam_step_ranges: [nr][2] int64 (first element, float4 groups before the range), and the element total."""
        pieces, _ = self.shard_plan()
        rows, pre = [], 0
        for a, n in pieces:
            assert a % 4 == 0 and n % 4 == 0, "arena segments are 256 B aligned and sharded chunks divide by 4 * world"
            rows.append((a, pre))
            pre += n // 4
        return torch.tensor(rows, dtype=torch.int64, device=device), len(rows), 4 * pre

    def sharded_grad_norm(self, grad):
        """2-norm of the rank-summed gradient after a SHARDED reduction (``clip_grad_norm`` with the sharded optimizer step): the squares
        of the pieces this rank owns plus 1 / world of the chunks every rank holds whole, summed over ranks in ONE inline fp64
        all-reduce.  Non-owned pieces of the arena (partial sums) are never read.  One host sync, like the unsharded clip."""
        _, chunks = self.shard_plan()
        W, r = self.shard_world, self.rank % self.shard_world
        own, whole = [], []
        for row in chunks:
            for a, b, sh in row:
                if sh:
                    n = (b - a) // W
                    own.append(grad[a + r * n:a + (r + 1) * n])
                else:
                    whole.append(grad[a:b])
        sq = lambda ts: torch.stack(torch._foreach_norm(ts)).double().square().sum() if ts else torch.zeros((), dtype=torch.float64,
                                                                                                            device=grad.device)
        t = (sq(own) + sq(whole) / self.world_size).reshape(1)
        self.all_reduce_sum(t)
        return float(t.sqrt())

    def gather_params(self, flat):
        """After Adam on the owned pieces: all-gather the sharded chunks of the parameter arena in FORWARD order (fc0 head, layers 0 ..
        L-1, tail) on the side stream, one mark per bucket; the next forward waits per bucket (``params_ready``)."""
        _, chunks = self.shard_plan()
        on_side = self.comm is not None and flat.is_cuda
        for bi in reversed(range(len(self.buckets))):
            for a, b, sh in chunks[bi]:
                if not sh:
                    continue
                if on_side:
                    self.comm.all_gather(flat[a:b])       # (a one-rank proxy group: a no-op plus the modelled transfer)
                else:
                    assert self.shard_world == self.world_size
                    n = (b - a) // self.world_size
                    dist.all_gather_into_tensor(flat[a:b], flat[a + self.rank * n:a + (self.rank + 1) * n].clone(), group=self.group)
            if on_side:
                self.comm.mark(bi)
        self._pending = on_side

    def params_ready(self, bucket):
        """The compute stream waits for the all-gather of bucket ``bucket`` (index into ``self.buckets``: 0 = tail, ``layer_bucket(l)``,
        L + 1 = the fc0 head).  No-op unless a sharded step left gathers in flight."""
        if self._pending and self.peer is not None:
            self.peer.params_wait()            # one flag round covers the whole arena: the forward's first per-bucket wait does it
            return
        if self._pending:
            self.comm.wait_mark(bucket)

    def params_ready_all(self):
        """Everything that reads the parameters outside a training forward (eval, checkpoints, tests) calls this first."""
        if self._pending:
            if self.peer is not None and self.peer.step_done:
                self.peer.params_wait()
            elif self.comm is not None:
                self.comm.wait()
            self._pending = False

    def peer_setup(self, flat, grad):
        """Build the peer-pointer exchange once the trainer's gradient arena exists (collective: every rank calls it)."""
        if self.peer is None:
            self.peer = PeerExchange(flat, grad, self.group)
        return self.peer

    def layer_bucket(self, l):
        return 1 + (self.model.n_layers - 1 - l)

    def _reduce(self, grad, s, e, big=False):
        if self._step_p2p:
            return
        for a, b in self.chunks(s, e):
            if self.comm is not None and grad.is_cuda:
                if self._step_sharded and self._sharded(a, b, big):
                    self.comm.reduce_scatter(grad[a:b])    # rank r keeps the sum of piece r; same side stream, same ordering
                else:
                    self.comm.enqueue(grad[a:b])           # rpb_dp_allreduce_enqueue: side stream, overlaps the rest of backward
            else:                                          # gloo (CPU tests) has no reduce-scatter: the all-reduce leaves the owner's piece equal
                self._works.append(dist.all_reduce(grad[a:b], op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def bucket_ready(self, grad, hold_small_of=None):
        """Called by the backward pass each time the next bucket (in ``self.buckets`` order) is complete.  ``hold_small_of`` = l: the
        bucket's tail from ``convs.l.weight`` on (the layer's Conv3d / BatchNorm gradients, 17 KB) is NOT final yet -- round 4 forms
        d convs.l.weight in the layer's data-gradient cell_mix, ~3 ms of kernels after the 100 MB spectral gradient -- and goes out
        with ``small_ready(grad, l)``; the spectral part starts its reduction now, as before."""
        bi = self._next
        self._next += 1
        for s, e, big in self.parts(bi):
            if hold_small_of is not None and not big and 1 <= bi <= self.model.n_layers:
                self._held[hold_small_of] = (s, e)
            else:
                self._reduce(grad, s, e, big)

    def small_ready(self, grad, l):
        """The held tail of layer ``l``'s bucket is complete: its own (tiny) all-reduce."""
        if l in self._held:
            self._reduce(grad, *self._held.pop(l))

    def finish_step(self, grad):
        while self._next < len(self.buckets):          # anything the backward pass did not announce
            self.bucket_ready(grad)
        for l in sorted(self._held, reverse=True):     # (same order on every rank)
            self._reduce(grad, *self._held.pop(l))
        if self.comm is not None and grad.is_cuda:
            self.comm.wait()                           # the compute stream (Adam next) waits for every bucket
        for w in self._works:
            w.wait()
        self._works = []

    def close(self):
        """Trainer teardown: destroy the RCCL communicators.  The wrapper stays attached to the model and is marked closed: a later
        step raises instead of silently training unsynchronised (round-3 advisor finding)."""
        if self.comm is not None:
            self.comm.close()
        if self.peer is not None:
            self.peer.close()
        self.closed = True

    def _live(self):
        if getattr(self, "closed", False):
            raise RuntimeError("DataParallel.close() was called: this model can no longer take synchronised steps "
                               "(build a new DataParallel, or set model.dp = None for single-process training)")

    # ---- sharding of a global batch / dataset index (replaces shuffle=True of train.py:269 under DP)
    def shard(self, n_items):
        per = n_items // self.world_size
        return range(self.rank * per, (self.rank + 1) * per)
