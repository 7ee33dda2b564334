#!/usr/bin/env python
"""WDNO measured on the MI355X at the cylinder shape ([20,64,128,3] -> [20,64,128,3], bior1.1, dim 256, dim_mults [1,2], 10 DDIM steps:
configs/cylinder/wdno.yaml, random weights, rescaler of ones): eval forward time per batch size and the per-launch HIP-event table of
one forward, split into ``rpb_conv7x``, the rest of the U-Net, and the wavelet and step kernels.  ``rpb_conv7x``'s issued bf16 MFMA rate
(six products per fp32 product) is stated against the rate rpb_mfma_probe sustains in the same run.  One number is arithmetic alone: the
bytes the im2col path would have moved for the init convolution -- that path is NOT run at this shape.
Launches under ~100 us are dominated by the event overhead in the table.
    python tools/wdno_probe.py [--batches 1 8] [--runs 5] [--out profiles/wdno_probe.txt]"""
import argparse
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from realpdebench_amd import _lib                          # noqa: E402
from realpdebench_amd import ops                           # noqa: E402
from realpdebench_amd.model import load_model             # noqa: E402

SHAPE = (20, 64, 128, 3)
DEV = "cuda:0"
CFG = dict(model_name="wdno", dim=256, dim_mults=[1, 2], wave_type="bior1.1", pad_mode="zero", beta_schedule="sigmoid",
           sampling_timesteps=10, ddim_sampling_eta=1)


def sustained_bf16():
    """The matrix rate this repository states its fractions against (bench.py mfma_ceiling, random operands), TFLOP/s."""
    seed, out = torch.randn(4096, device=DEV), torch.empty(256 * 2 * 512, device=DEV)
    ops.mfma_probe(seed, out, 2000)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fl = ops.mfma_probe(seed, out, 40000)
    e1.record()
    torch.cuda.synchronize()
    return fl / (e0.elapsed_time(e1) * 1e9)


class One(torch.utils.data.Dataset):
    def __len__(self):
        return 1

    def __getitem__(self, i):
        return torch.zeros(*SHAPE), torch.zeros(*SHAPE)


def group_of(label):
    if label.startswith("conv7x["):
        return "rpb_conv7x"
    if label.startswith("wdno_"):
        return "wavelet + step kernels"
    return "rest of the U-Net"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    root = tempfile.mkdtemp()
    os.makedirs(os.path.join(root, "d"))
    torch.save(torch.ones(1, 1, 1, 1, 48), os.path.join(root, "d", "wdno_rescaler_bior1.1_zero.pt"))
    torch.manual_seed(0)
    m = load_model(One(), device=DEV, dataset_root=root, dataset_name="d", **CFG).eval()
    Tp, Hp, Wp = m.padded_shape
    cells, Ci, N, K = Tp * Hp * Wp, m.channels, m.model.dim, 343 * m.channels
    say(f"WDNO cylinder shape {SHAPE}, bior1.1: coefficient mesh {m.coef_shape} padded to {m.padded_shape} = {cells} cells per sample, "
        f"{Ci} state channels, U-Net dim {N}, {m.sampling_timesteps} DDIM steps")
    ldc = (K + 127) // 128 * 128
    say(f"init_conv as im2col + GEMM (NOT run at this shape; arithmetic only): column matrix {cells} x {ldc} fp32 = {cells * ldc * 4 / 1e9:.2f} GB "
        f"per sample, written once and read once per sampling step = {2 * cells * ldc * 4 * m.sampling_timesteps / 1e9:.1f} GB per sample and "
        f"forward; at test_batch_size 64: {cells * ldc * 4 * 64 / 1e9:.0f} GB resident")
    peak = sustained_bf16()
    say(f"sustained bf16 MFMA rate of this chip (rpb_mfma_probe, random operands): {peak:.0f} TFLOP/s")
    for B in a.batches:
        x = torch.randn(B, *SHAPE, device=DEV)
        with torch.no_grad():
            m(x)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.runs):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                m(x)
                e.record()
                torch.cuda.synchronize()
                ts.append(s.elapsed_time(e))
            med = statistics.median(ts)
            say(f"B={B}: eval forward ({m.sampling_timesteps} U-Net forwards) median {med:.2f} ms over {a.runs} runs after 1 warm-up (min {min(ts):.2f}, "
                f"max {max(ts):.2f}); {B / med * 1e3:.2f} samples/s")
            _lib.PROFILE = {}
            m(x)
            torch.cuda.synchronize()
            prof = _lib.profile_summary()
            _lib.PROFILE = None
        groups = {}
        for label, r in prof.items():
            g = groups.setdefault(group_of(label), dict(calls=0, ms=0.0))
            g["calls"] += r["calls"]
            g["ms"] += r["total_ms"]
        tot = sum(g["ms"] for g in groups.values())
        say(f"  HIP-event table (one forward, sum {tot:.2f} ms incl. event overhead)")
        say(f"  {'group':<26}{'calls':>6}{'total ms':>10}{'share':>7}")
        for name, g in sorted(groups.items(), key=lambda kv: -kv[1]["ms"]):
            say(f"  {name:<26}{g['calls']:>6}{g['ms']:>10.3f}{g['ms'] / tot:>7.2f}")
        c7 = [r for label, r in prof.items() if label.startswith("conv7x[")][0]
        fl = 2.0 * B * cells * N * K
        say(f"  rpb_conv7x [N{N},Ci{Ci},K7] M={B * cells}: {c7['avg_ms']:.3f} ms per call ({c7['calls']} calls); fp32-grade {fl / c7['avg_ms'] / 1e9:.1f} "
            f"TFLOP/s delivered; issued {6 * fl / c7['avg_ms'] / 1e9:.0f} TFLOP/s bf16 MFMA = {6 * fl / c7['avg_ms'] / 1e9 / peak:.2f} of the sustained "
            f"rate of this run")
        top = sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"])[:8]
        for label, r in top:
            say(f"    {label:<34}{r['calls']:>5}{r['total_ms']:>10.3f} ms")
        del x
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
