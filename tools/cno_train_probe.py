#!/usr/bin/env python
"""The opt-in CNO3d training step measured on the MI355X at the cylinder shape: one ``ArenaTrainer.step`` per batch size (median of 10
after 3 warm-ups), the eval forward of the same run next to it, the per-launch HIP-event table by kernel family (the ``label``s of
model/cno.py and ops.py), the share of the new row kernels (csrc/rpb_rowbn.hip) and ``torch.cuda.max_memory_allocated``.
Launches under ~100 us are dominated by the event overhead in the table.
    python tools/cno_train_probe.py [--batches 1 2 4] [--runs 10] [--out profiles/cno_train_probe.txt]
``--sync-bn``: what SyncBN costs a rank (``sync_vs_plain`` below), instead of the table.
    python tools/cno_train_probe.py --sync-bn [--batches 1 2 4] [--runs 5] [--repeats 3] [--out profiles/cno_syncbn_probe.txt]"""
import argparse
import os
import re
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from realpdebench_amd import _lib                         # noqa: E402
from realpdebench_amd.model.cno import CNO3d              # noqa: E402
from realpdebench_amd.trainer import make_trainer         # noqa: E402
from tools.cno_probe import DEV, HBM_PEAK, SHAPE, median_ms          # noqa: E402

ROW_KERNELS = ("rowbn_stats", "rowbn_finish", "rowbn_act_fwd", "rowbn_act_bwd_stats", "rowbn_sum64", "rowbn_act_bwd_apply")


def family(label):
    """conv3x_wgrad[Co64,Ci128] -> conv3x_wgrad: one row per kernel, whatever the shape"""
    return re.sub(r"\[.*\]$", "", label)


def sync_vs_plain(title, new_model, shape, batches, runs, repeats, backend):
    """The syncing step against the plain step of the same process, on a one-rank process group with RPB_DP_SYNCBN_ALWAYS=1: the syncing
    instance (``enable_training(sync_bn=True)``) then runs every launch of the N-rank step -- per BatchNorm layer one more rowbn_sum64, the
    finish from sums, a copy of the backward sums and two all-reduces over one rank -- but no byte crosses a link.  Per batch size the
    two steps are timed alternately, ``repeats`` times each (median of ``runs`` after 3 warm-ups); reported: the median of those medians
    and their spread (min .. max).  ``new_model(**enable_training arguments)`` builds an enabled instance on the device."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    os.environ["RPB_DP_SYNCBN_ALWAYS"] = "1"
    dist.init_process_group(backend, rank=0, world_size=1)
    lines = [f"{title}, shape {shape}: SyncBN step against the plain step, one process, one-rank {backend} group, RPB_DP_SYNCBN_ALWAYS=1",
             "(the one-rank proxy: every launch of the N-rank step, no link traffic; no run with more than one rank on RCCL has taken place)"]
    trs = {}
    try:
        torch.manual_seed(0)
        plain, sync = new_model(), new_model(sync_bn=True)
        trs["plain"], trs["sync"] = make_trainer(plain, lr=1e-4, num_update=10000), make_trainer(sync, lr=1e-4, num_update=10000)
        assert plain.bn_sync is None and sync.bn_sync is not None and sync.bn_sync.sync_stats_always
        lines.append(f"reductions: {'RCCL through the C ABI (rpb_dp_allreduce_inline)' if sync.bn_sync.comm is not None else 'torch.distributed'}")
        for B in batches:
            x, y = torch.randn(B, *shape, device=DEV), torch.randn(B, *shape, device=DEV)
            meds = {"plain": [], "sync": []}
            for _ in range(repeats):
                for k in ("sync", "plain"):
                    meds[k].append(median_ms(lambda: trs[k].step(x, y), runs)[0])
            mp, ms = statistics.median(meds["plain"]), statistics.median(meds["sync"])
            lines.append(f"B={B}: plain step {mp:.2f} ms (medians {min(meds['plain']):.2f} .. {max(meds['plain']):.2f}); syncing step {ms:.2f} ms "
                         f"(medians {min(meds['sync']):.2f} .. {max(meds['sync']):.2f}); sync - plain = {ms - mp:+.2f} ms = {(ms - mp) / mp:+.4f} "
                         f"of the plain step; {repeats} alternating repeats of the median of {runs} runs after 3 warm-ups")
            del x, y
            torch.cuda.empty_cache()
    finally:
        for tr in trs.values():
            tr.close()
        dist.destroy_process_group()
    return lines


def emit(lines, out):
    txt = "\n".join(lines)
    print(txt)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(txt + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--runs", type=int, default=None, help="default 10; 5 with --sync-bn")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sync-bn", action="store_true", help="time the SyncBN step against the plain step (sync_vs_plain)")
    ap.add_argument("--repeats", type=int, default=3, help="--sync-bn: alternating repeats of each median")
    ap.add_argument("--backend", default="nccl", help="--sync-bn: backend of the one-rank process group")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cno_train_probe.py measures on an MI355X: no GPU, no number")
    if a.sync_bn:
        new = lambda **kw: CNO3d(in_dim=SHAPE[-1], in_size=SHAPE[1], N_layers=3, out_dim=SHAPE[-1]).to(DEV).enable_training(**kw)
        return emit(sync_vs_plain("CNO3d N_layers = 3, opt-in training step (ArenaTrainer.step)", new, SHAPE, a.batches, a.runs or 5, a.repeats,
                                  a.backend), a.out)
    a.runs = a.runs or 10
    torch.manual_seed(0)
    m = CNO3d(in_dim=SHAPE[-1], in_size=SHAPE[1], N_layers=3, out_dim=SHAPE[-1]).to(DEV).enable_training()
    tr = make_trainer(m, lr=1e-4, num_update=10000)
    lines = [f"CNO3d N_layers = 3, opt-in training step (ArenaTrainer.step), shape {SHAPE}"]
    for B in a.batches:
        x, y = torch.randn(B, *SHAPE, device=DEV), torch.randn(B, *SHAPE, device=DEV)
        with torch.no_grad():
            ev = median_ms(lambda: m.eval()(x), a.runs)
        torch.cuda.reset_peak_memory_stats()
        med, lo, hi = median_ms(lambda: tr.step(x, y), a.runs)
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        lines.append(f"B={B}: training step median {med:.2f} ms over {a.runs} runs after 3 warm-ups (min {lo:.2f}, max {hi:.2f}); eval forward of "
                     f"this run {ev[0]:.2f} ms; step / eval forward = {med / ev[0]:.2f}; max_memory_allocated {peak:.2f} GiB")
        _lib.PROFILE = {}
        tr.step(x, y)
        torch.cuda.synchronize()
        fam = {}
        for k, v in _lib.profile_summary().items():
            f = fam.setdefault(family(k), dict(calls=0, ms=0.0, gb=0.0, tf=0.0))
            f["calls"] += v["calls"]
            f["ms"] += v["total_ms"]
            f["gb"] += v["bytes"] * v["calls"] / 1e9
            f["tf"] += v["flops"] * v["calls"] / 1e12
        _lib.PROFILE = None
        tot = sum(v["ms"] for v in fam.values())
        rows = sum(v["ms"] for k, v in fam.items() if k in ROW_KERNELS)
        lines.append(f"  HIP-event table (one step, sum {tot:.2f} ms incl. event overhead; torch's own launches -- allocation fills, layout "
                     f"permutes, the loss -- are not in it); new row kernels {rows:.2f} ms = {rows / tot:.3f} of the sum")
        lines.append(f"  {'family':<26}{'calls':>6}{'total ms':>10}{'share':>7}{'GB':>9}{'of 8 TB/s':>11}{'TFLOP/s':>9}")
        for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"]):
            t = v["ms"] * 1e-3
            lines.append(f"  {k:<26}{v['calls']:>6}{v['ms']:>10.3f}{v['ms'] / tot:>7.2f}{v['gb']:>9.3f}{v['gb'] * 1e9 / t / HBM_PEAK:>11.3f}"
                         f"{v['tf'] / t:>9.2f}")
        del x, y
        torch.cuda.empty_cache()
    emit(lines, a.out)


if __name__ == "__main__":
    main()
