"""Galerkin Transformer eval forward at the cylinder config ([B,20,64,128,3], configs/cylinder/galerkin_transformer.yaml) on one MI355X:
GalerkinTransformer3d.set_arith("f16x2") against the default arithmetic, alternately in one process on the same seeded input.
  1. rpb_gemm3h against the default token GEMM on the same operands at the production shapes M = B 163840, (N, K) = (768, 256) bias,
     (256, 256) bias + ReLU, (256, 256) bias + residual, (128, 256) plain; the issued fp16 MFMA rate of rpb_gemm3h (three products per
     fp32 product) against the rate rpb_mfma_probe sustains in the same run.  Each side is timed as the forward runs it: the default is
     ops.gemm_nt WITH its per-call weight preparation, rpb_gemm3h reads planes prepared once (they are cached in the model).  The
     default's preparation is also timed alone and printed, so that the part of a difference that is preparation can be read off -- at
     B = 1 it is of the size of the spread.
  2. The whole eval forward for each B: the default, set_arith("f16x2") as shipped (``F16X2_SITES``) and set_arith("f16x2") with all four
     GEMMs routed to rpb_gemm3h, alternately; medians of ``--runs`` runs after 3 warm-ups, ``--repeats`` alternating repeats (the spread
     of a configuration is the range of its medians), a HIP-event table per kernel family, the share of the four GEMMs, and the Rel-L2 of
     each f16x2 output against the default's.
``--default-only`` runs part 2 for the default arithmetic alone (no use of set_arith): the same script measures a checkout without the
switch, e.g. the parent commit, in the same session (``--root`` names that checkout, ``--label`` what the output calls it).
    python tools/galerkin_probe.py [--batches 1 4 16] [--runs 20] [--repeats 2] [--default-only] [--root DIR] [--label TEXT]
                                   [--out profiles/galerkin_arith_probe.txt]"""
import argparse
import os
import statistics
import sys

import torch
import yaml

HBM_PEAK = 8.0e12
GEMMS = ("gemm3h", "gemm3x", "gemm_nt")          # label prefixes of the token GEMM launches (weight preparation: *_wprep)


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


def sustained_bf16(ops):
    """The matrix rate this repository states its fractions against (bench.py mfma_ceiling, random operands), TFLOP/s."""
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
    for key in ("gemm3h_wprep", "gemm3x_wprep") + GEMMS:
        if label.startswith(key):
            return key
    return label.split("[")[0]


def family_table(_lib, m, x, lines, name):
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
    lines.append(f"  HIP-event table, {name} (one forward, sum {tot:.3f} ms incl. event overhead)")
    lines.append(f"  {'family':<26}{'calls':>6}{'total ms':>10}{'share':>7}{'GB':>9}{'of 8 TB/s':>11}{'TFLOP/s':>9}")
    for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"]):
        t = max(v["ms"], 1e-6) * 1e-3
        lines.append(f"  {k:<26}{v['calls']:>6}{v['ms']:>10.3f}{v['ms'] / tot:>7.2f}{v['bytes'] / 1e9:>9.3f}{v['bytes'] / t / HBM_PEAK:>11.3f}"
                     f"{v['flops'] / t / 1e12:>9.2f}")
    g = sum(v["ms"] for k, v in fam.items() if k in GEMMS or k.endswith("_wprep"))
    lines.append(f"  token GEMMs (with weight preparation) {g:.3f} ms = {g / tot:.2f} of the forward")
    return fam, tot


def gemm_compare(_lib, ops, B, runs, repeats, sustained, lines):
    M, C = B * 163840, 256
    gen = torch.Generator(device="cuda:0").manual_seed(100 + B)
    A = torch.randn(M, C, device="cuda:0", generator=gen)
    A *= torch.exp2(torch.randint(-6, 7, (M, 1), device="cuda:0", generator=gen).float())        # rows of different binades, as after residual adds
    res = torch.randn(M, C, device="cuda:0", generator=gen)
    for name, N, bias, act, residual in (("Q|K|V", 768, True, 0, False), ("lr1", 256, True, 3, False), ("lr2", 256, True, 0, True), ("fc", 128, False, 0, False)):
        W = torch.randn(N, C, device="cuda:0", generator=gen) / 16
        b = torch.randn(N, device="cuda:0", generator=gen) if bias else None
        r = res if residual else None
        out0, out1 = torch.empty(M, N, device="cuda:0"), torch.empty(M, N, device="cuda:0")
        wz = ops.gemm3h_wprep(W)
        f0 = lambda: ops.gemm_nt(A, W, out0, M, N, C, bias=b, residual=r, act=act)
        f1 = lambda: ops.gemm_nt_f16x2(A, wz, out1, M, N, C, bias=b, residual=r, act=act)
        wz3 = torch.empty(3 * N * C, dtype=torch.int16, device="cuda:0")
        fp = lambda: _lib.call("rpb_gemm3x_wprep", ops._p(W), ops._p(wz3, torch.int16), N, C, ops._stream())     # what ops.gemm_nt runs per call
        t0, t1 = [], []
        for _ in range(repeats):
            t0.append(median_ms(f0, runs))
            t1.append(median_ms(f1, runs))
        prep = median_ms(fp, runs)
        m0, m1 = statistics.median(t0), statistics.median(t1)
        spread = max(max(t0) - min(t0), max(t1) - min(t1))
        want = A.double() @ W.double().t()
        if b is not None:
            want += b.double()
        if act == 3:
            want.relu_()
        if r is not None:
            want += r.double()
        e0, e1 = (float((o.double() - want).norm() / want.norm()) for o in (out0, out1))
        del want
        issued = 2.0 * M * N * C * 3 / (m1 * 1e-3) / 1e12
        byts = 4.0 * M * (C + N * (2 if residual else 1))
        lines.append(f"B={B} {name} M={M} N={N} K={C}: default " + " ".join(f"{t:.3f}" for t in t0) + " ms, gemm3h " + " ".join(f"{t:.3f}" for t in t1)
                     + f" ms (medians of {runs}); {m0:.3f} -> {m1:.3f} ms ({m0 / m1:.3f}x), spread {spread:.3f} ms: "
                     + ("faster" if m0 - m1 > spread else "NOT faster by more than the spread")
                     + f" (the default's time includes its weight preparation, alone {prep:.3f} ms; without it {(m0 - prep) / m1:.3f}x)"
                     + f"; gemm3h {issued:.0f} TFLOP/s issued fp16 MFMA = {issued / sustained:.2f} of the sustained rate of this run ({sustained:.0f}, bf16 probe), "
                     f"{byts / (m1 * 1e-3) / HBM_PEAK:.2f} of 8 TB/s; Rel-L2 against fp64: default {e0:.2e}, gemm3h {e1:.2e}")
        del out0, out1
    del A, res
    torch.cuda.empty_cache()


def forward_compare(_lib, m, B, shape, runs, repeats, default_only, lines):
    x = torch.randn(B, *shape, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(B))
    ariths = ("f32",) if default_only else ("f32", "f16x2", "f16x2 all four")

    def select(a):
        if default_only:
            return m
        m.__dict__.pop("F16X2_SITES", None)                            # back to the class's routing
        if a == "f16x2 all four":
            m.F16X2_SITES = type(m).ALL_F16X2_SITES
        return m.set_arith("f32" if a == "f32" else "f16x2")

    meds = {a: [] for a in ariths}
    errs = {}
    with torch.no_grad():
        for _ in range(repeats):
            for a in ariths:
                select(a)
                meds[a].append(median_ms(lambda: m(x), runs))
        if not default_only:
            want = select("f32")(x).double()
            errs = {a: float((select(a)(x).double() - want).norm() / want.norm()) for a in ariths[1:]}
            del want
    med = {k: statistics.median(v) for k, v in meds.items()}
    spread = max(max(v) - min(v) for v in meds.values())
    for k, v in meds.items():
        lines.append(f"B={B} {k}: eval forward medians of {runs} runs after 3 warm-ups, {repeats} alternating repeats: "
                     + " ".join(f"{t:.3f}" for t in v) + f" ms; median {med[k]:.3f} ms, spread {max(v) - min(v):.3f} ms; {B / med[k] * 1e3:.1f} samples/s")
    for k in ariths[1:]:
        gain = med["f32"] - med[k]
        lines.append(f"B={B}: f32 - {k} = {gain:.3f} ms ({med['f32'] / med[k]:.3f}x); largest spread {spread:.3f} ms: "
                     + ("faster" if gain > spread else "NOT faster by more than the spread")
                     + f"; Rel-L2 of the output against the default's on the same seeded input {errs[k]:.2e}")
    for a in ariths:
        family_table(_lib, select(a), x, lines, a)
    select("f32")
    del x
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this checkout", help="what the output's first line calls the checkout under --root")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/galerkin_probe.py measures on an MI355X: no GPU, no number")
    sys.path.insert(0, os.path.abspath(a.root))
    from realpdebench_amd import _lib, ops
    from realpdebench_amd.model import load_model
    with open(os.path.join(a.root, "realpdebench_amd", "configs", "cylinder", "galerkin_transformer.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    shape_in, shape_out = tuple(cfg["shape_in"]), tuple(cfg["shape_out"])

    class One(torch.utils.data.Dataset):
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return torch.zeros(*shape_in), torch.zeros(*shape_out)

    torch.manual_seed(0)
    m = load_model(One(), device="cuda:0", **cfg).eval()
    sustained = sustained_bf16(ops)
    lines = [f"GalerkinTransformer3d, cylinder config, shape {shape_in}, {a.label} (its {os.path.relpath(_lib.LIB_PATH, os.path.abspath(a.root))})"
             + (": the default arithmetic alone" if a.default_only else ": set_arith('f16x2') against the default arithmetic, alternately in one process"),
             f"sustained bf16 MFMA rate of this chip (rpb_mfma_probe, random operands): {sustained:.0f} TFLOP/s"]
    if not a.default_only:
        for B in a.batches:
            gemm_compare(_lib, ops, B, a.runs, a.repeats, sustained, lines)
    for B in a.batches:
        forward_compare(_lib, m, B, shape_in, a.runs, a.repeats, a.default_only, lines)
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.default_only else "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
