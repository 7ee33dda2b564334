#!/usr/bin/env python
"""CNO3d measured on the MI355X at the cylinder shape: eval forward time per batch size, the per-launch HIP-event table (the ``label``s
of model/cno.py), the 128 -> 128 layer's issued bf16 MFMA rate against the rate rpb_mfma_probe measures in the same run, and the fused
launch (rpb_cno_conv3x writing fp32 rows + bf16 planes) against the two passes it replaces (rpb_conv3x + rpb_split3) at the same shape.
Launches under ~100 us are dominated by the event overhead in the table.
``--arith f16x2`` measures CNO3d.set_arith("f16x2") instead: both arithmetics alternately in this process on the same seeded input (the
default path is the comparison; the spread is what repeating one configuration gives), the HIP-event table of each, the 128 -> 128
layer's issued fp16 MFMA rate, the share of the split passes and the Rel-L2 of the f16x2 output against the default's.
    python tools/cno_probe.py [--arith f32|f16x2] [--batches 1 8] [--runs 20] [--repeats 3] [--out profiles/cno_probe.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from realpdebench_amd import _lib, ops                    # noqa: E402
from realpdebench_amd.model.cno import CNO3d              # noqa: E402

HBM_PEAK = 8.0e12
SHAPE = (20, 64, 128, 3)
DEV = "cuda:0"


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


def median_ms(fn, runs, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts), min(ts), max(ts)


def fused_vs_pair(C, B, runs, sustained):
    """One C -> C layer at the cylinder mesh: rpb_cno_conv3x (fp32 + planes out) against rpb_conv3x followed by rpb_split3."""
    T, H, W = SHAPE[:3]
    M = B * T * H * W
    g = torch.Generator(device=DEV).manual_seed(C)
    x = torch.randn(M, C, device=DEV, generator=g)
    w = torch.randn(C, 27 * C, device=DEV, generator=g) / (27 * C) ** 0.5
    sc, sh = torch.rand(C, device=DEV, generator=g) + 0.5, torch.randn(C, device=DEV, generator=g)
    planes = torch.empty(3 * M * C, dtype=torch.int16, device=DEV)
    ops.split3(x, planes, M, C)
    wz = CNO3d.k_wprep(w, C, C)
    out, op = torch.empty(M, C, device=DEV), torch.empty(3 * M * C, dtype=torch.int16, device=DEV)
    fused = median_ms(lambda: CNO3d.k_conv(planes, wz, sc, sh, M, C, C, (T, H, W), C, 1, out=out, ldo=C, out_planes=op, ldp=C), runs)
    conv = median_ms(lambda: ops.conv3x(planes, wz, out, M, C, C, (T, H, W), bias=sh), runs)
    split = median_ms(lambda: ops.split3(out, op, M, C), runs)
    # v_mfma_f32_32x32x16_bf16 per launch: 128-token tiles x 27 taps x 16-channel chunks x (4 x N / 32) output tiles x six products
    mf = -(-M // 128) * 27 * (C // 16) * 6 * 4 * (C // 32)
    issued = mf * 32768 / (fused[0] * 1e-3) / 1e12
    useful = 2.0 * M * C * 27 * C / (fused[0] * 1e-3) / 1e12
    return [f"  {C:>3} -> {C:<3} B={B} M={M}: rpb_cno_conv3x (fp32 + planes out) median {fused[0]:.3f} ms (min {fused[1]:.3f}); "
            f"rpb_conv3x {conv[0]:.3f} + rpb_split3 {split[0]:.3f} = {conv[0] + split[0]:.3f} ms; fused / pair = {fused[0] / (conv[0] + split[0]):.3f}",
            f"             issued {issued:.0f} TFLOP/s bf16 MFMA = {issued / sustained:.2f} of the sustained rate of this run ({sustained:.0f} TFLOP/s); "
            f"fp32-grade {useful:.1f} TFLOP/s delivered"]


def event_table(m, x, lines):
    """one forward under HIP events -> {label: summary}; the table is appended to ``lines``"""
    with torch.no_grad():
        _lib.PROFILE = {}
        m(x)
        torch.cuda.synchronize()
    fam = _lib.profile_summary()
    _lib.PROFILE = None
    tot = sum(v["total_ms"] for v in fam.values())
    lines.append(f"  HIP-event table, arith = {m.arith} (one forward, sum {tot:.3f} ms incl. event overhead; allocation and zero-fill are not launches of this table)")
    lines.append(f"  {'family':<32}{'calls':>6}{'total ms':>10}{'share':>7}{'GB':>9}{'of 8 TB/s':>11}{'TFLOP/s':>9}")
    for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["total_ms"]):
        t = v["total_ms"] * 1e-3
        lines.append(f"  {k:<32}{v['calls']:>6}{v['total_ms']:>10.3f}{v['total_ms'] / tot:>7.2f}{v['bytes'] * v['calls'] / 1e9:>9.3f}"
                     f"{v['bytes'] * v['calls'] / t / HBM_PEAK:>11.3f}{v['flops'] * v['calls'] / t / 1e12:>9.2f}")
    return fam, tot


def arith_compare(m, B, runs, repeats, sustained, lines):
    """f32 and f16x2 alternately, ``repeats`` times each: the spread of a configuration is the range of its medians."""
    T, H, W = SHAPE[:3]
    M = B * T * H * W
    x = torch.randn(B, *SHAPE, device=DEV, generator=torch.Generator(device=DEV).manual_seed(B))
    meds = {"f32": [], "f16x2": []}
    with torch.no_grad():
        for _ in range(repeats):
            for arith in ("f32", "f16x2"):
                m.set_arith(arith)
                meds[arith].append(median_ms(lambda: m(x), runs)[0])
        want = m.set_arith("f32")(x)
        got = m.set_arith("f16x2")(x)
        err = float((got.double() - want.double()).norm() / want.double().norm())
        del want, got
    med = {k: statistics.median(v) for k, v in meds.items()}
    spread = {k: max(v) - min(v) for k, v in meds.items()}
    gain = med["f32"] - med["f16x2"]
    for k in ("f32", "f16x2"):
        lines.append(f"B={B} arith={k}: eval forward medians of {runs} runs after 3 warm-ups, {repeats} alternating repeats: "
                     + " ".join(f"{t:.3f}" for t in meds[k]) + f" ms; median {med[k]:.3f} ms, spread {spread[k]:.3f} ms; {B / med[k] * 1e3:.2f} samples/s")
    lines.append(f"B={B}: f32 - f16x2 = {gain:.3f} ms ({med['f32'] / med['f16x2']:.3f}x); largest spread {max(spread.values()):.3f} ms: "
                 + ("f16x2 is faster by more than the spread" if gain > max(spread.values()) else "f16x2 is NOT faster by more than the spread"))
    lines.append(f"B={B}: Rel-L2 of the f16x2 output against the default's on the same seeded input: {err:.2e}")
    for arith in ("f32", "f16x2"):
        fam, tot = event_table(m.set_arith(arith), x, lines)
    passes = sum(v["total_ms"] for k, v in fam.items() if k in ("split2h", "amax_exp_finish", "cno_pack_f16x2"))
    lines.append(f"  split passes (split2h + amax_exp_finish + cno_pack_f16x2): {passes:.3f} ms = {passes / tot:.3f} of the f16x2 table; "
                 f"split2h moves {fam['split2h']['bytes'] * fam['split2h']['calls'] / 1e9:.3f} GB")
    v = fam["cno_conv3x_f16x2[N128,Ci128]"]
    # v_mfma_f32_32x32x16_f16 per launch: 128-token tiles x 27 taps x 16-channel chunks x (4 x N / 32) output tiles x three products
    mf = -(-M // 128) * 27 * (128 // 16) * 3 * 4 * (128 // 32)
    issued = mf * 32768 / (v["avg_ms"] * 1e-3) / 1e12
    lines.append(f"  128 -> 128 layer: {v['avg_ms']:.3f} ms per launch; issued {issued:.0f} TFLOP/s fp16 MFMA = {issued / sustained:.2f} of the sustained "
                 f"rate of this run ({sustained:.0f} TFLOP/s, rpb_mfma_probe); fp32-grade {2.0 * M * 128 * 27 * 128 / (v['avg_ms'] * 1e-3) / 1e12:.1f} TFLOP/s delivered")
    m.set_arith("f32")
    del x
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3, help="with --arith f16x2: alternating repeats of each arithmetic")
    ap.add_argument("--arith", default="f32", choices=["f32", "f16x2"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cno_probe.py measures on an MI355X: no GPU, no number")
    torch.manual_seed(0)
    m = CNO3d(in_dim=SHAPE[-1], in_size=SHAPE[1], N_layers=3, out_dim=SHAPE[-1]).to(DEV).eval()
    sustained = sustained_bf16()
    if a.arith == "f16x2":
        lines = [f"CNO3d N_layers = 3, shape {SHAPE}: set_arith('f16x2') against the default arithmetic, alternately in one process",
                 f"sustained bf16 MFMA rate of this chip (rpb_mfma_probe, random operands): {sustained:.0f} TFLOP/s"]
        for B in a.batches:
            arith_compare(m, B, a.runs, a.repeats, sustained, lines)
        txt = "\n".join(lines)
        print(txt)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(txt + "\n")
        return
    cells = SHAPE[0] * SHAPE[1] * SHAPE[2]
    lines = [f"CNO3d N_layers = 3, shape {SHAPE} ({cells} cells per sample, 15.85 MFLOP useful per cell = {15.85e6 * cells / 1e12:.2f} TFLOP per sample)",
             f"sustained bf16 MFMA rate of this chip (rpb_mfma_probe, random operands): {sustained:.0f} TFLOP/s"]
    for B in a.batches:
        x = torch.randn(B, *SHAPE, device=DEV)
        with torch.no_grad():
            med, lo, hi = median_ms(lambda: m(x), a.runs)
            lines.append(f"B={B}: eval forward median {med:.3f} ms over {a.runs} runs after 3 warm-ups (min {lo:.3f}, max {hi:.3f}); "
                         f"{B / med * 1e3:.2f} samples/s; {15.85e6 * cells * B / (med * 1e-3) / 1e12:.1f} TFLOP/s useful")
            _lib.PROFILE = {}
            m(x)
            torch.cuda.synchronize()
        fam = _lib.profile_summary()
        _lib.PROFILE = None
        tot = sum(v["total_ms"] for v in fam.values())
        lines.append(f"  HIP-event table (one forward, sum {tot:.3f} ms incl. event overhead; allocation and zero-fill of the plane buffers are not launches of this table)")
        lines.append(f"  {'family':<26}{'calls':>6}{'total ms':>10}{'share':>7}{'GB':>9}{'of 8 TB/s':>11}{'TFLOP/s':>9}")
        for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["total_ms"]):
            t = v["total_ms"] * 1e-3
            lines.append(f"  {k:<26}{v['calls']:>6}{v['total_ms']:>10.3f}{v['total_ms'] / tot:>7.2f}{v['bytes'] * v['calls'] / 1e9:>9.3f}"
                         f"{v['bytes'] * v['calls'] / t / HBM_PEAK:>11.3f}{v['flops'] * v['calls'] / t / 1e12:>9.2f}")
        del x
        torch.cuda.empty_cache()
    lines.append("fused launch against the passes it replaces (same shape, same run; median of %d after 3 warm-ups)" % a.runs)
    for C in (64, 128):
        lines += fused_vs_pair(C, 1, a.runs, sustained)
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
