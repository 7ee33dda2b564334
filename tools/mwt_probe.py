"""MWT3d eval forward at the cylinder shape on one MI355X: median time over >= 20 runs for B = 1, 8, 32 and a per-family kernel table
from HIP events (algorithmic bytes and FLOPs of each launch are the bookkeeping of model/mwt.py).  Launches under ~100 us are dominated
by the event overhead in this table: take those from `rocprofv3 --kernel-trace --stats -- python tools/mwt_probe.py
--no-events` instead.
``--arith`` selects MWT3d.set_arith (f32 = the default path; bf16x3 / f16x2 = the split-operand convolutions).
    python tools/mwt_probe.py [--arith f32|bf16x3|f16x2] [--batches 1 8 32] [--runs 20] [--no-events] [--out profiles/mwt_probe.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from realpdebench_amd import _lib                         # noqa: E402
from realpdebench_amd.model.mwt import MWT3d              # noqa: E402

HBM_PEAK, COPY_CEIL = 8.0e12, (5.2e12, 6.0e12)           # B/s: data-sheet peak; the copy ceiling measured in this repository
SHAPE = (20, 64, 128, 3)


def sustained_bf16():
    """The matrix rate this repository states its convolution fractions against (bench.py mfma_ceiling, random operands), TFLOP/s."""
    from realpdebench_amd import ops
    seed, out = torch.randn(4096, device="cuda:0"), torch.empty(256 * 2 * 512, device="cuda:0")
    ops.mfma_probe(seed, out, 2000)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fl = ops.mfma_probe(seed, out, 40000)
    e1.record()
    torch.cuda.synchronize()
    return fl / (e0.elapsed_time(e1) * 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-events", action="store_true")
    ap.add_argument("--arith", default="f32", choices=["f32", "bf16x3", "f16x2"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mwt_probe.py measures on an MI355X: no GPU, no number")
    torch.manual_seed(0)
    m = MWT3d(k=3, alpha=5, c=4, nCZ=4, L=0, base="legendre", shape_in=SHAPE, shape_out=SHAPE).to("cuda:0").eval()
    m.set_arith(a.arith)
    lines = [f"arith = {a.arith}"]
    sustained = sustained_bf16()
    fl_rate = lambda v: v["flops"] * v["calls"] / (v["total_ms"] * 1e-3) / 1e12
    lines.append(f"sustained bf16 MFMA rate of this chip (rpb_mfma_probe, random operands): {sustained:.0f} TFLOP/s")
    for B in a.batches:
        x = torch.randn(B, *SHAPE, device="cuda:0")
        with torch.no_grad():
            for _ in range(3):
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
        lines.append(f"B={B}: eval forward median {med:.3f} ms over {a.runs} runs (min {min(ts):.3f}, max {max(ts):.3f}); "
                     f"{B / med * 1e3:.1f} samples/s")
        if a.no_events:
            continue
        _lib.PROFILE = {}
        with torch.no_grad():
            m(x)
        torch.cuda.synchronize()
        summ = _lib.profile_summary()
        _lib.PROFILE = None
        tot = sum(v["total_ms"] for v in summ.values())
        stream_bytes = sum(v["bytes"] * v["calls"] for v in summ.values())
        lines.append(f"  HIP-event table (one forward, sum {tot:.3f} ms incl. event overhead; algorithmic bytes {stream_bytes / 1e9:.2f} GB = "
                     f"{stream_bytes / COPY_CEIL[1] * 1e3:.2f}-{stream_bytes / COPY_CEIL[0] * 1e3:.2f} ms at the 5.2-6.0 TB/s copy ceiling)")
        lines.append(f"  {'family':<16}{'calls':>6}{'total ms':>10}{'GB':>9}{'of 8 TB/s':>11}{'TFLOP/s':>9}")
        for k, v in sorted(summ.items(), key=lambda kv: -kv[1]["total_ms"]):
            by, fl, t = v["bytes"] * v["calls"], v["flops"] * v["calls"], v["total_ms"] * 1e-3
            lines.append(f"  {k:<16}{v['calls']:>6}{v['total_ms']:>10.3f}{by / 1e9:>9.3f}{by / t / HBM_PEAK:>11.3f}{fl / t / 1e12:>9.2f}")
        fam = {k: v for k, v in summ.items() if k.startswith("mwt_conv3") or k == "mwt_amax_exp"}
        if fam:
            lines.append(f"  mwt_conv3 family ({' + '.join(sorted(fam))}): {sum(v['total_ms'] for v in fam.values()):.3f} ms")
        label = "mwt_conv3" if a.arith == "f32" else f"mwt_conv3[{a.arith}]"
        if label in summ:
            v = summ[label]
            cells = v["flops"] * v["calls"] / (2 * (27 * 36 + 36) * 36)
            # per 64 cells (12 tiles of the 48-row padded output); Lo is 12 * 12 v_mfma_f32_16x16x4_f32 in every mode
            lo_mf, lo_fl = cells / 64 * 12 * 12, 16 * 16 * 4 * 2
            if a.arith == "f32":
                # one v_mfma_f32_16x16x4_f32 = 16 * 16 * 4 * 2 FLOP; 27 taps x 9 steps
                mf, per, name, ceil_, what = cells / 64 * 27 * 9 * 12, 2048, "16x16x4 f32", sustained / 16, "fp32 MFMA ceiling (sustained bf16 rate / 16)"
            else:
                # one v_mfma_f32_16x16x32_{bf16,f16} = 16 * 16 * 32 * 2 FLOP; 31 steps of the flat K = 992, 6 or 3 products each
                prod = 6 if a.arith == "bf16x3" else 3
                mf, per, name, ceil_, what = (cells / 64 * 31 * 12 * prod, 16384, "16x16x32 bf16" if prod == 6 else "16x16x32 f16", sustained,
                                              "sustained bf16 rate")
            issued = (mf * per + lo_mf * lo_fl) / (v["total_ms"] * 1e-3) / 1e12
            lines.append(f"  {label}: {mf:.3e} MFMA ({name}) + {lo_mf:.3e} (16x16x4 f32, Lo) = {issued:.1f} TFLOP/s issued; the main product alone "
                         f"= {mf * per / (v['total_ms'] * 1e-3) / 1e12 / ceil_:.2f} of the {what} ({sustained:.0f} TFLOP/s measured here with random "
                         f"operands); useful rows 36/48.  fp32-grade FLOP/s delivered {fl_rate(v):.1f} TFLOP/s; conv3x's split-bf16 (3 products per "
                         f"fp32-grade product) at its documented 0.75-0.86 of the sustained rate delivers {0.75 * sustained / 3:.0f}-"
                         f"{0.86 * sustained / 3:.0f}")
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
