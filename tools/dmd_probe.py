"""DMD forward at B = 12 (the YAMLs' test_batch_size) for the five native shapes on one MI355X, split into its three parts: the Gram
kernel pair (HIP events), the host solve (numpy, wall clock; fed the Gram matrices the kernel produced) and the predict kernel (HIP
events), next to the wall clock of the whole forward (copies and the one synchronisation included).  Each figure is the median of
``--runs`` runs after 3 warm-ups, repeated ``--repeats`` times: the spread is the range of those medians.  The effective bandwidth of
a kernel is its algorithmic traffic (whole C-wide cells of the frames it reads, plus what it writes) over its median time, against
8 TB/s.  Nothing here is a pass/fail threshold.  Inputs are N(0,1) (the synthetic default).
    python tools/dmd_probe.py [--batch 12] [--runs 20] [--repeats 3] [--out profiles/dmd_probe.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from realpdebench_amd import ops                                          # noqa: E402
from realpdebench_amd.model.dmd import DMD, dmd_coefficients              # noqa: E402

HBM_PEAK = 8.0e12
SCENARIOS = ("cylinder", "controlled_cylinder", "fsi", "foil", "combustion")


def event_ms(fn, runs, warm=3):
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


def wall_ms(fn, runs, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def fmt(vals):
    return f"{statistics.median(vals):8.3f} ms (spread {max(vals) - min(vals):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmd_probe.txt"))
    a = ap.parse_args()
    B = a.batch
    lines = [f"DMD forward, B = {B}, {torch.cuda.get_device_name(0)}; medians of {a.runs} runs after 3 warm-ups, {a.repeats} repeats "
             "(spread = range of the medians)"]
    for scen in SCENARIOS:
        with open(os.path.join(ROOT, "realpdebench_amd", "configs", scen, "dmd.yaml")) as fh:
            cfg = yaml.safe_load(fh)
        T, H, W, C = cfg["shape_in"]
        f, S = cfg["input_feature"], cfg["n_predict"]
        m = DMD(cfg["n_modes"], S, f, 1, cfg["shape_in"], cfg["shape_out"]).to("cuda:0")
        x = torch.from_numpy(np.random.default_rng(7).standard_normal((B, T, H, W, C), dtype=np.float32)).to("cuda:0")
        x4 = x.view(B, T, H * W, C)
        G = ops.dmd_gram(x4, f).cpu().numpy()
        Md = torch.from_numpy(dmd_coefficients(G, H * W * f, m.n_modes, S)).to("cuda:0")
        gram, host, pred, fwd = [], [], [], []
        for _ in range(a.repeats):
            gram.append(event_ms(lambda: ops.dmd_gram(x4, f), a.runs))
            ts = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                dmd_coefficients(G, H * W * f, m.n_modes, S)
                ts.append((time.perf_counter() - t0) * 1e3)
            host.append(statistics.median(ts))
            pred.append(event_ms(lambda: ops.dmd_predict(x4, Md, f), a.runs))
            fwd.append(wall_ms(lambda: m(x), a.runs))
        gb = 4 * B * T * H * W * C
        pb = 4 * B * (T - 1) * H * W * C + 4 * B * S * H * W * f
        g, p = statistics.median(gram) * 1e-3, statistics.median(pred) * 1e-3
        lines += [f"{scen}: x [{B},{T},{H},{W},{C}], f = {f}, n_predict = {S}",
                  f"  gram (2 launches)  {fmt(gram)}   {gb / 1e6:8.1f} MB -> {gb / g / 1e12:.2f} TB/s = {gb / g / HBM_PEAK:.2f} of 8 TB/s",
                  f"  host solve         {fmt(host)}   {B} eigenproblems of order {T - 1}",
                  f"  predict            {fmt(pred)}   {pb / 1e6:8.1f} MB -> {pb / p / 1e12:.2f} TB/s = {pb / p / HBM_PEAK:.2f} of 8 TB/s",
                  f"  whole forward      {fmt(fwd)}   wall clock, copies and synchronisation included; {B / statistics.median(fwd) * 1e3:.0f} samples/s"]
    with open(os.path.join(ROOT, "tests", "golden", "dmd_configs.json")) as fh:
        ref = json.load(fh)["reference_cpu_seconds_per_sample"]
    lines.append(f"reference on the CPU of the fixture generator's host, cylinder shape: {min(ref['runs']):.3f}-{max(ref['runs']):.3f} s per sample "
                 "(tests/golden/dmd_configs.json; another machine, not measured in this run)")
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt)


if __name__ == "__main__":
    main()
