"""DPOT eval forward at configs/cylinder/dpot_s.yaml and dpot_l.yaml ([B,20,128,128,2]) on one MI355X: DPOT.set_arith("f16x2") against
the default arithmetic, alternately in one process on the same seeded input.
  1. Per site of ``DPOT.ALL_F16X2_SITES``: rpb_gemm3hk (rpb_afno_mlp_f16x2 for "afno") against the default kernel on the same operands at
     the shape the config gives the site for each B -- mlp0 (bias + GELU), mlp2 (bias + residual), out0 (bias + GELU), out2 (bias +
     GELU), tagg (plain), afno.  Each side is timed as the forward runs it: the default is ops.gemm_nt WITH its per-call weight
     preparation (ops.afno_mlp with its two ops.afno_wprep), the f16x2 kernels read planes prepared once (the model caches them); the
     row-exponent pre-pass of rpb_gemm3hk is inside its time and is also timed alone ("rowexp").  Medians of ``--runs`` runs after 2
     warm-ups, ``--repeats`` alternating repeats; the spread is the range of a side's medians; a site counts as faster only if the
     difference of the medians exceeds the larger spread.  A shape the kernel refuses is listed as such.
  2. The whole eval forward for each config and B: the default, set_arith("f16x2") as shipped (``F16X2_SITES``) and with every wired
     site on, alternately; a HIP-event table per launch label, and the Rel-L2 of each f16x2 output against the default's.
    python tools/dpot_probe.py [--configs dpot_s dpot_l] [--batches 16 64] [--runs 7] [--repeats 2] [--out profiles/dpot_arith_probe.txt]"""
import argparse
import os
import statistics
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def median_ms(fn, runs, warm=2):
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


def alternate(f0, f1, runs, repeats):
    t0, t1 = [], []
    for _ in range(repeats):
        t0.append(median_ms(f0, runs))
        t1.append(median_ms(f1, runs))
    m0, m1 = statistics.median(t0), statistics.median(t1)
    spread = max(max(t0) - min(t0), max(t1) - min(t1))
    return t0, t1, m0, m1, spread


def site_shapes(cfg, B):
    """{site: (M, N, K, bias, act, residual)} as DPOT._forward_hip runs them"""
    E, ps, T = cfg["embed_dim"], cfg["patch_size"], cfg["in_timesteps"]
    n = cfg["img_size"] // ps
    hid, OD = int(E * cfg["mlp_ratio"]), cfg["out_layer_dim"]
    E1p = (cfg["out_channels"] * ps + 3 + 31) // 32 * 32
    Mt = B * n * n
    return {"mlp0": (Mt, hid, E, True, 1, False), "mlp2": (Mt, E, hid, True, 0, True), "out0": (Mt, ps * ps * OD, E, True, 1, False),
            "out2": (Mt * ps * ps, OD, OD, True, 1, False), "tagg": (Mt, E, T * E1p, False, 0, False)}


def gemm_sites(ops, name, cfg, B, runs, repeats, lines, verdict):
    gen = torch.Generator(device=DEV).manual_seed(100 + B)
    for site, (M, N, K, bias, act, residual) in site_shapes(cfg, B).items():
        tag = f"{name} B={B} {site} M={M} N={N} K={K}"
        if not ops.gemm3hk_supported(M, N, K):
            lines.append(f"{tag}: refused by rpb_gemm3hk_supported, stays on the default kernel")
            continue
        A = torch.randn(M, K, device=DEV, generator=gen)
        A *= torch.exp2(torch.randint(-6, 7, (M, 1), device=DEV, generator=gen).float())      # rows of different binades, as after residual adds
        W = torch.randn(N, K, device=DEV, generator=gen) / K ** 0.5
        b = torch.randn(N, device=DEV, generator=gen) if bias else None
        r = torch.randn(M, N, device=DEV, generator=gen) if residual else None
        out0, out1 = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
        rowe = torch.empty(M, dtype=torch.int32, device=DEV)
        wz = ops.gemm3h_wprep(W)
        f0 = lambda: ops.gemm_nt(A, W, out0, M, N, K, bias=b, residual=r, act=act)
        f1 = lambda: ops.gemm_nt_f16x2k(A, wz, out1, M, N, K, bias=b, residual=r, act=act)
        t0, t1, m0, m1, spread = alternate(f0, f1, runs, repeats)
        pre = median_ms(lambda: ops.gemm3hk_rowexp(A, rowe, M, K), runs)
        rows = min(M, 2048)                                            # the error on a slab of rows: fp64 of the whole product is not needed
        want = A[:rows].double() @ W.double().t()
        if b is not None:
            want += b.double()
        if act == 1:
            want = torch.nn.functional.gelu(want)
        if r is not None:
            want += r[:rows].double()
        e0, e1 = (float((o[:rows].double() - want).norm() / want.norm()) for o in (out0, out1))
        issued = 2.0 * M * N * K * 3 / (m1 * 1e-3) / 1e12
        fast = m0 - m1 > spread
        verdict.setdefault(site, []).append((f"{name} B={B}", fast, m0 / m1))
        lines.append(f"{tag}: default " + " ".join(f"{t:.3f}" for t in t0) + " ms, gemm3hk " + " ".join(f"{t:.3f}" for t in t1)
                     + f" ms (medians of {runs}); {m0:.3f} -> {m1:.3f} ms ({m0 / m1:.3f}x), spread {spread:.3f} ms: "
                     + ("faster" if fast else "NOT faster by more than the spread")
                     + f"; rowexp alone {pre:.3f} ms ({pre / m1:.3f} of the call); {issued:.0f} TFLOP/s issued fp16 MFMA; "
                     f"Rel-L2 against fp64 on {rows} rows: default {e0:.2e}, gemm3hk {e1:.2e}")
        del A, W, b, r, out0, out1, want, wz
        torch.cuda.empty_cache()


def afno_site(ops, name, cfg, B, runs, repeats, lines, verdict):
    E, nb = cfg["embed_dim"], cfg["n_blocks"]
    bs, n = E // nb, cfg["img_size"] // cfg["patch_size"]
    ntok = B * min(cfg["modes"], n) * min(cfg["modes"], n // 2 + 1)
    tag = f"{name} B={B} afno ntok={ntok} nb={nb} bs={bs}"
    if not ops.afno_f16x2_supported(nb, bs):
        lines.append(f"{tag}: refused by rpb_afno_mlp_f16x2_supported, stays on the default kernel")
        return
    gen = torch.Generator(device=DEV).manual_seed(200 + B)
    X = torch.randn(ntok, 2, E, device=DEV, generator=gen) * torch.exp2(torch.randint(-10, 11, (ntok, 1, 1), device=DEV, generator=gen).float())
    w1, w2 = (torch.randn(2, nb, bs, bs, device=DEV, generator=gen) / bs ** 0.5 for _ in range(2))
    b1, b2 = (0.1 * torch.randn(2, nb, bs, device=DEV, generator=gen) for _ in range(2))
    o0, o1 = torch.empty(ntok, 2 * E, device=DEV), torch.empty(ntok, 2 * E, device=DEV)
    W1c, W2c = torch.empty(nb, 2 * bs, 2 * bs, device=DEV), torch.empty(nb, 2 * bs, 2 * bs, device=DEV)
    w1z, w2z = ops.afno_wprep_f16x2(w1, nb, bs), ops.afno_wprep_f16x2(w2, nb, bs)

    def f0():
        ops.afno_wprep(w1, W1c, nb, bs, False)
        ops.afno_wprep(w2, W2c, nb, bs, False)
        ops.afno_mlp(X, W1c, b1, W2c, b2, None, None, o0, ntok, nb, bs, 0)

    f1 = lambda: ops.afno_mlp_f16x2(X, w1z, b1, w2z, b2, o1, ntok, nb, bs)
    t0, t1, m0, m1, spread = alternate(f0, f1, runs, repeats)
    fast = m0 - m1 > spread
    verdict.setdefault("afno", []).append((f"{name} B={B}", fast, m0 / m1))
    d = float((o1.double() - o0.double()).norm() / o0.double().norm())
    lines.append(f"{tag}: default " + " ".join(f"{t:.3f}" for t in t0) + " ms, afno_mlp_f16x2 " + " ".join(f"{t:.3f}" for t in t1)
                 + f" ms (medians of {runs}); {m0:.3f} -> {m1:.3f} ms ({m0 / m1:.3f}x), spread {spread:.3f} ms: "
                 + ("faster" if fast else "NOT faster by more than the spread") + f"; Rel-L2 against the default kernel {d:.2e}")


def label_table(_lib, m, x, lines, name):
    _lib.PROFILE = {}
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()
    rows = _lib.profile_summary()
    _lib.PROFILE = None
    tot = sum(v["total_ms"] for v in rows.values())
    lines.append(f"  HIP-event table, {name} (one forward, sum {tot:.3f} ms incl. event overhead; labels below 1 % of it are summed as 'other')")
    lines.append(f"  {'label':<34}{'calls':>6}{'total ms':>10}{'share':>7}{'TFLOP/s':>9}")
    other = 0.0
    for k, v in sorted(rows.items(), key=lambda kv: -kv[1]["total_ms"]):
        if v["total_ms"] < 0.01 * tot:
            other += v["total_ms"]
            continue
        t = max(v["total_ms"], 1e-6) * 1e-3
        lines.append(f"  {k:<34}{v['calls']:>6}{v['total_ms']:>10.3f}{v['total_ms'] / tot:>7.2f}{v['flops'] * v['calls'] / t / 1e12:>9.1f}")
    lines.append(f"  {'other':<34}{'':>6}{other:>10.3f}{other / tot:>7.2f}")


def forward_compare(_lib, m, name, B, shape, runs, repeats, lines):
    x = torch.randn(B, *shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(B))
    ariths = ("f32", "f16x2", "f16x2 every site")

    def select(a):
        m.__dict__.pop("F16X2_SITES", None)                            # back to the class's routing
        if a == "f16x2 every site":
            m.F16X2_SITES = type(m).ALL_F16X2_SITES
        return m.set_arith("f32" if a == "f32" else "f16x2")

    meds = {a: [] for a in ariths}
    with torch.no_grad():
        for _ in range(repeats):
            for a in ariths:
                select(a)
                meds[a].append(median_ms(lambda: m(x), runs))
        want = select("f32")(x).double()
        errs, ran = {}, {}
        for a in ariths[1:]:
            errs[a] = float((select(a)(x).double() - want).norm() / want.norm())
            ran[a] = m.f16x2_ran
        del want
    med = {k: statistics.median(v) for k, v in meds.items()}
    spread = max(max(v) - min(v) for v in meds.values())
    for k, v in meds.items():
        lines.append(f"{name} B={B} {k}: eval forward medians of {runs} runs after 2 warm-ups, {repeats} alternating repeats: "
                     + " ".join(f"{t:.3f}" for t in v) + f" ms; median {med[k]:.3f} ms, spread {max(v) - min(v):.3f} ms; {B / med[k] * 1e3:.1f} samples/s")
    for k in ariths[1:]:
        gain = med["f32"] - med[k]
        lines.append(f"{name} B={B}: f32 - {k} = {gain:.3f} ms ({med['f32'] / med[k]:.3f}x); largest spread {spread:.3f} ms: "
                     + ("faster" if gain > spread else "NOT faster by more than the spread")
                     + f"; sites on the new kernels {ran[k]}; Rel-L2 of the output against the default's on the same seeded input {errs[k]:.2e}")
    for a in ariths:
        label_table(_lib, select(a), x, lines, f"{name} B={B} {a}")
    select("f32")
    del x
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["dpot_s", "dpot_l"])
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--no-forward", action="store_true", help="part 1 only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dpot_probe.py measures on an MI355X: no GPU, no number")
    sys.path.insert(0, ROOT)
    from realpdebench_amd import _lib, ops
    from realpdebench_amd.model import load_model
    from realpdebench_amd.model.dpot import DPOT
    lines = [f"DPOT, cylinder configs: set_arith('f16x2') against the default arithmetic, alternately in one process; shipped F16X2_SITES = "
             f"{DPOT.F16X2_SITES} of {DPOT.ALL_F16X2_SITES}"]
    verdict = {}

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    for name in a.configs:
        with open(os.path.join(ROOT, "realpdebench_amd", "configs", "cylinder", name + ".yaml")) as fh:
            cfg = yaml.safe_load(fh)
        shape_in, shape_out = tuple(cfg["shape_in"]), tuple(cfg["shape_out"])
        for B in a.batches:
            n0 = len(lines)
            gemm_sites(ops, name, cfg, B, a.runs, a.repeats, lines, verdict)
            afno_site(ops, name, cfg, B, a.runs, a.repeats, lines, verdict)
            print("\n".join(lines[n0:]), flush=True)
            flush()
        if a.no_forward:
            continue

        class One(torch.utils.data.Dataset):
            def __len__(self):
                return 1

            def __getitem__(self, i):
                return torch.zeros(*shape_in), torch.zeros(*shape_out)

        torch.manual_seed(0)
        m = load_model(One(), device=DEV, **cfg).eval()
        for B in a.batches:
            n0 = len(lines)
            forward_compare(_lib, m, name, B, shape_in, a.runs, a.repeats, lines)
            print("\n".join(lines[n0:]), flush=True)
            flush()
        del m
        torch.cuda.empty_cache()
    lines.append("per site, over the shapes above (faster = by more than the spread of the same run):")
    for site, rows in verdict.items():
        lines.append(f"  {site}: " + ", ".join(f"{w} {'faster' if f else 'not faster'} {r:.3f}x" for w, f, r in rows))
    print("\n".join(lines[-1 - len(verdict):]))
    flush()


if __name__ == "__main__":
    main()
