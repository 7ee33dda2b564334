#!/usr/bin/env python
"""The opt-in DeepONet training step measured on the MI355X at the cylinder shape (p = 128, dropout 0.1): one ``ArenaTrainer.step`` per
batch size (median of 10 after 3 warm-ups), the eval forward of the same run next to it, the per-launch HIP-event table by kernel
family (the ``label``s of model/deeponet.py, model/_common.py and ops.py), the share of the new row kernels
(csrc/rpb_deeponet_train.hip and the BatchNorm backward tail of csrc/rpb_rowbn.hip) and ``torch.cuda.max_memory_allocated``.  Launches under ~100 us are dominated by the event overhead in
the table.  No speed threshold: the step / forward ratio is recorded, not asserted.
    python tools/deeponet_train_probe.py [--batches 1 4] [--runs 10] [--out profiles/deeponet_train_probe.txt]
``--sync-bn``: what SyncBN costs a rank (``tools.cno_train_probe.sync_vs_plain``), instead of the table.
    python tools/deeponet_train_probe.py --sync-bn [--batches 1 4] [--runs 5] [--repeats 3] [--out profiles/deeponet_syncbn_probe.txt]"""
import argparse
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from realpdebench_amd import _lib                         # noqa: E402
from realpdebench_amd.model.deeponet import DeepONet      # noqa: E402
from realpdebench_amd.trainer import make_trainer         # noqa: E402
from tools.cno_probe import DEV, HBM_PEAK, median_ms      # noqa: E402
from tools.cno_train_probe import emit, sync_vs_plain     # noqa: E402
from tools.deeponet_probe import P, SHAPE                 # noqa: E402

ROW_KERNELS = ("don_pool_bwd", "rowbn_sum64", "rowbn_act_bwd_apply", "don_point_mul", "don_point_mul_bwd")


def family(label):
    """don_gemm3x[N512,K128] -> don_gemm3x: one row per kernel, whatever the shape"""
    return re.sub(r"\[.*\]$", "", label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--runs", type=int, default=None, help="default 10; 5 with --sync-bn")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sync-bn", action="store_true", help="time the SyncBN step against the plain step (sync_vs_plain)")
    ap.add_argument("--repeats", type=int, default=3, help="--sync-bn: alternating repeats of each median")
    ap.add_argument("--backend", default="nccl", help="--sync-bn: backend of the one-rank process group")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/deeponet_train_probe.py measures on an MI355X: no GPU, no number")
    if a.sync_bn:
        new = lambda **kw: DeepONet(SHAPE, SHAPE, SHAPE[-1], SHAPE[-1], P, dropout_rate=0.1).to(DEV).enable_training(**kw)
        return emit(sync_vs_plain(f"DeepONet p = {P}, dropout 0.1, opt-in training step (ArenaTrainer.step)", new, SHAPE, a.batches, a.runs or 5,
                                  a.repeats, a.backend), a.out)
    a.runs = a.runs or 10
    torch.manual_seed(0)
    m = DeepONet(SHAPE, SHAPE, SHAPE[-1], SHAPE[-1], P, dropout_rate=0.1).to(DEV).enable_training()
    tr = make_trainer(m, lr=1e-4, num_update=10000)
    lines = [f"DeepONet p = {P}, dropout 0.1, opt-in training step (ArenaTrainer.step), shape {SHAPE}, output net in chunks of {m._point_rows} rows"]
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
        lines.append(f"  HIP-event table (one step, sum {tot:.2f} ms incl. event overhead; torch's own launches -- allocation fills, slice "
                     f"copies, the loss -- are not in it); new row kernels {rows:.2f} ms = {rows / tot:.3f} of the sum")
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
