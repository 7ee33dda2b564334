"""DeepONet eval forward at the cylinder shape (p = 128) on one MI355X: median time over 20 runs after 3 warm-ups for B = 1, 8, 64 (64 is
the YAML's test_batch_size), a per-family kernel table from HIP events (algorithmic bytes and FLOPs of each launch are the bookkeeping
of model/deeponet.py) and the point-MLP kernel's issued bf16 MFMA rate against the rate rpb_mfma_probe measures in the same run.
Launches under ~100 us are dominated by the event overhead in this table.
``--arith f16x2`` measures DeepONet.set_arith("f16x2") instead: the default arithmetic, the f16x2 output net alone (``F16X2_SITES = ("point",)``) and
the f16x2 output net with branch stages 2-4 on the f16x2 convolution, alternately in this process on the same seeded input (the default
path is the comparison; the spread is what repeating one configuration gives), the HIP-event table of each, the point kernel's issued
fp16 MFMA rate (three products per fp32 product) and the Rel-L2 of the f16x2 output against the default's.
    python tools/deeponet_probe.py [--arith f32|f16x2] [--batches 1 8 64] [--runs 20] [--repeats 2] [--no-events]
                                   [--out profiles/deeponet_probe.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from realpdebench_amd import _lib                         # noqa: E402
from realpdebench_amd.model.deeponet import DeepONet      # noqa: E402

HBM_PEAK = 8.0e12
SHAPE, P = (20, 64, 128, 3), 128


def sustained_bf16():
    """The matrix rate this repository states its fractions against (bench.py mfma_ceiling, random operands), TFLOP/s."""
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


def family(label):
    for key in ("don_point_mlp_f16x2", "don_point_mlp", "conv3x_f16x2", "don_trunk", "don_bn_relu_pool", "don_conv3x", "don_split3", "don_im2col", "don_gemm3x"):
        if label.startswith(key):
            return key
    return label


CONFIGS = (("f32", "f32", ("point", "convs")), ("f16x2 point", "f16x2", ("point",)), ("f16x2 point+conv", "f16x2", ("point", "convs")))


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
    return statistics.median(ts)


def family_table(m, x, lines, name):
    """one forward (trunk cached) under HIP events -> {family: sums}; the table is appended to ``lines``"""
    _lib.PROFILE = {}
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()
    fam = {}
    for label, v in _lib.profile_summary().items():
        f = fam.setdefault(family(label), dict(calls=0, ms=0.0, bytes=0.0, flops=0.0))
        f["calls"] += v["calls"]
        f["ms"] += v["total_ms"]
        f["bytes"] += v["bytes"] * v["calls"]
        f["flops"] += v["flops"] * v["calls"]
    _lib.PROFILE = None
    tot = sum(v["ms"] for v in fam.values())
    lines.append(f"  HIP-event table, {name} (one forward, trunk cached, sum {tot:.3f} ms incl. event overhead)")
    lines.append(f"  {'family':<22}{'calls':>6}{'total ms':>10}{'share':>7}{'GB':>9}{'of 8 TB/s':>11}{'TFLOP/s':>9}")
    for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"]):
        t = v["ms"] * 1e-3
        lines.append(f"  {k:<22}{v['calls']:>6}{v['ms']:>10.3f}{v['ms'] / tot:>7.2f}{v['bytes'] / 1e9:>9.3f}{v['bytes'] / t / HBM_PEAK:>11.3f}"
                     f"{v['flops'] / t / 1e12:>9.2f}")
    return fam, tot


def arith_compare(m, B, runs, repeats, sustained, lines):
    """The three configurations alternately, ``repeats`` times each: the spread of a configuration is the range of its medians."""
    x = torch.randn(B, *SHAPE, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(B))
    N = SHAPE[0] * SHAPE[1] * SHAPE[2]

    def select(cfg):
        m.set_arith(cfg[1])
        m.F16X2_SITES = cfg[2]
        return m

    meds = {c[0]: [] for c in CONFIGS}
    with torch.no_grad():
        for _ in range(repeats):
            for cfg in CONFIGS:
                select(cfg)
                meds[cfg[0]].append(median_ms(lambda: m(x), runs))
        want = select(CONFIGS[0])(x)
        errs = {c[0]: float((select(c)(x).double() - want.double()).norm() / want.double().norm()) for c in CONFIGS[1:]}
        del want
    med = {k: statistics.median(v) for k, v in meds.items()}
    spread = max(max(v) - min(v) for v in meds.values())
    for k, v in meds.items():
        lines.append(f"B={B} {k}: eval forward medians of {runs} runs after 3 warm-ups, {repeats} alternating repeats: "
                     + " ".join(f"{t:.3f}" for t in v) + f" ms; median {med[k]:.3f} ms, spread {max(v) - min(v):.3f} ms; {B / med[k] * 1e3:.1f} samples/s")
    for k in list(med)[1:]:
        gain = med["f32"] - med[k]
        lines.append(f"B={B}: f32 - {k} = {gain:.3f} ms ({med['f32'] / med[k]:.3f}x); largest spread {spread:.3f} ms: "
                     + ("a gain (more than three times the spread)" if gain > 3 * spread else "NOT a gain by the three-spread rule")
                     + f"; Rel-L2 against the default output on the same seeded input {errs[k]:.2e}")
    d = med["f16x2 point"] - med["f16x2 point+conv"]
    lines.append(f"B={B}: stages 2-4 on the f16x2 convolution change the f16x2 forward by {-d:+.3f} ms (spread {spread:.3f} ms)")
    tables = {}
    for cfg in CONFIGS:
        tables[cfg[0]] = family_table(select(cfg), x, lines, cfg[0])
    conv = lambda fam, keys: sum(fam[k]["ms"] for k in keys if k in fam)
    lines.append(f"  conv3x family of stages 2-4: default don_split3 + don_conv3x {conv(tables['f32'][0], ('don_split3', 'don_conv3x')):.3f} ms; "
                 f"f16x2 amax_exp + split2h + conv3x_f16x2 {conv(tables['f16x2 point+conv'][0], ('amax_exp', 'split2h', 'conv3x_f16x2')):.3f} ms")
    steps = B * -(-N // 128) * 4 * (16 * (P // 16 + 8) + 8)                # k-steps of all wave tiles, one MFMA per product
    for name, key, products, pipe in (("f32", "don_point_mlp", 6, "bf16"), ("f16x2 point", "don_point_mlp_f16x2", 3, "fp16")):
        v = tables[name][0][key]
        issued = steps * products * 32768 / (v["ms"] * 1e-3) / 1e12
        lines.append(f"  {key}: {v['ms']:.3f} ms; {steps * products:.3e} MFMA (32x32x16 {pipe}, {products} per fp32 product: issued = "
                     f"{products}x useful) = {issued:.0f} TFLOP/s issued = {issued / sustained:.2f} of the sustained rate of this run "
                     f"({sustained:.0f} TFLOP/s, rpb_mfma_probe, bf16); fp32-grade {v['flops'] / (v['ms'] * 1e-3) / 1e12:.1f} TFLOP/s delivered")
    select(CONFIGS[0])
    del m.F16X2_SITES
    del x
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arith", default="f32", choices=["f32", "f16x2"])
    ap.add_argument("--repeats", type=int, default=2, help="with --arith f16x2: alternating repeats of each configuration")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--no-events", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/deeponet_probe.py measures on an MI355X: no GPU, no number")
    torch.manual_seed(0)
    m = DeepONet(SHAPE, SHAPE, SHAPE[-1], SHAPE[-1], P).to("cuda:0").eval()
    sustained = sustained_bf16()
    lines = [f"DeepONet p = {P}, shape {SHAPE}; trunk output cached after the first call",
             f"sustained bf16 MFMA rate of this chip (rpb_mfma_probe, random operands): {sustained:.0f} TFLOP/s"]
    if a.arith == "f16x2":
        lines[0] = f"DeepONet p = {P}, shape {SHAPE}: set_arith('f16x2') against the default arithmetic, alternately in one process"
        for B in a.batches:
            arith_compare(m, B, a.runs, a.repeats, sustained, lines)
        a.batches = []
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
        m._layouts.invalidate()                      # the table shows the trunk launch once, as a first call would
        with torch.no_grad():
            m(x)
        torch.cuda.synchronize()
        fam = {}
        for label, v in _lib.profile_summary().items():
            f = fam.setdefault(family(label), dict(calls=0, ms=0.0, bytes=0.0, flops=0.0))
            f["calls"] += v["calls"]
            f["ms"] += v["total_ms"]
            f["bytes"] += v["bytes"] * v["calls"]
            f["flops"] += v["flops"] * v["calls"]
        _lib.PROFILE = None
        tot = sum(v["ms"] for v in fam.values())
        lines.append(f"  HIP-event table (one forward incl. the trunk launch, sum {tot:.3f} ms incl. event overhead)")
        lines.append(f"  {'family':<18}{'calls':>6}{'total ms':>10}{'share':>7}{'GB':>9}{'of 8 TB/s':>11}{'TFLOP/s':>9}")
        for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"]):
            t = v["ms"] * 1e-3
            lines.append(f"  {k:<18}{v['calls']:>6}{v['ms']:>10.3f}{v['ms'] / tot:>7.2f}{v['bytes'] / 1e9:>9.3f}{v['bytes'] / t / HBM_PEAK:>11.3f}"
                         f"{v['flops'] / t / 1e12:>9.2f}")
        if "don_point_mlp" in fam:
            v = fam["don_point_mlp"]
            N = SHAPE[0] * SHAPE[1] * SHAPE[2]
            # per 32-point wave tile: 16 blocks x (p / 16 + 8) k-steps + 8 of layer 3 (C_out padded to 32 rows), six products each,
            # one v_mfma_f32_32x32x16_bf16 = 32 * 32 * 16 * 2 FLOP
            mf = B * -(-N // 128) * 4 * (16 * (P // 16 + 8) + 8) * 6
            issued = mf * 32768 / (v["ms"] * 1e-3) / 1e12
            lines.append(f"  don_point_mlp: {mf:.3e} MFMA (32x32x16 bf16) = {issued:.0f} TFLOP/s issued = {issued / sustained:.2f} of the sustained "
                         f"bf16 rate measured in this run ({sustained:.0f} TFLOP/s); fp32-grade FLOP/s delivered {v['flops'] / (v['ms'] * 1e-3) / 1e12:.1f} "
                         f"TFLOP/s; share of the forward {v['ms'] / tot:.2f}")
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
