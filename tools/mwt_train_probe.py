#!/usr/bin/env python
"""The opt-in MWT3d training step measured on the MI355X at the cylinder shape [B, 20, 64, 128, 3], nCZ = 4: one ``ArenaTrainer.step``
per batch size (median of 20 after 3 warm-ups), the eval forward of the same run next to it, the per-launch HIP-event table by kernel
family (the ``label``s of model/mwt.py and ops.py), the two convolution-gradient kernels against the forward ``mwt_conv3`` family of the
same step (the same cells) and ``torch.cuda.max_memory_allocated``.  A batch size that does not fit is reported as such.
Launches under ~100 us are dominated by the event overhead in the table.
    python tools/mwt_train_probe.py [--batches 1 8 32] [--runs 20] [--out profiles/mwt_train_probe.txt]"""
import argparse
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from realpdebench_amd import _lib                         # noqa: E402
from realpdebench_amd.model.mwt import MWT3d              # noqa: E402
from realpdebench_amd.trainer import make_trainer         # noqa: E402
from tools.cno_probe import DEV, HBM_PEAK, SHAPE, median_ms          # noqa: E402


def family(label):
    return re.sub(r"\[.*\]$", "", label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mwt_train_probe.py measures on an MI355X: no GPU, no number")
    torch.manual_seed(0)
    m = MWT3d(k=3, alpha=5, c=4, nCZ=4, L=0, base="legendre", shape_in=SHAPE, shape_out=SHAPE).to(DEV).enable_training()
    tr = make_trainer(m, lr=1e-4, num_update=10000)
    lines = [f"MWT3d k = 3, alpha = 5, c = 4, nCZ = 4, opt-in training step (ArenaTrainer.step), shape {SHAPE}"]
    for B in a.batches:
        x, y = torch.randn(B, *SHAPE, device=DEV), torch.randn(B, *SHAPE, device=DEV)
        with torch.no_grad():
            ev = median_ms(lambda: m.eval()(x), a.runs)
        torch.cuda.reset_peak_memory_stats()
        try:
            med, lo, hi = median_ms(lambda: tr.step(x, y), a.runs)
        except torch.OutOfMemoryError:
            lines.append(f"B={B}: the training step does not fit (eval forward {ev[0]:.2f} ms)")
            del x, y
            torch.cuda.empty_cache()
            continue
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        lines.append(f"B={B}: training step median {med:.2f} ms over {a.runs} runs after 3 warm-ups (min {lo:.2f}, max {hi:.2f}); eval forward of "
                     f"this run {ev[0]:.2f} ms; step / eval forward = {med / ev[0]:.2f}; max_memory_allocated {peak:.2f} GiB "
                     f"({peak / B:.3f} GiB per sample)")
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
        fwd = fam.get("mwt_conv3", {"ms": float("nan")})["ms"]
        lines.append(f"  HIP-event table (one step, sum {tot:.2f} ms incl. event overhead; torch's own launches -- T0, the gates, the loss -- are "
                     f"not in it); against the forward mwt_conv3 family of this step ({fwd:.2f} ms, the same cells): "
                     + ", ".join(f"{k} {fam[k]['ms'] / fwd:.2f}x" for k in ("mwt_conv3_dgrad", "mwt_conv3_wgrad") if k in fam))
        lines.append(f"  {'family':<26}{'calls':>6}{'total ms':>10}{'share':>7}{'GB':>9}{'of 8 TB/s':>11}{'TFLOP/s':>9}")
        for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"]):
            t = v["ms"] * 1e-3
            lines.append(f"  {k:<26}{v['calls']:>6}{v['ms']:>10.3f}{v['ms'] / tot:>7.2f}{v['gb']:>9.3f}{v['gb'] * 1e9 / t / HBM_PEAK:>11.3f}"
                         f"{v['tf'] / t:>9.2f}")
        del x, y
        torch.cuda.empty_cache()
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
