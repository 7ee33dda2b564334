#!/usr/bin/env python
"""bench.py -- headline benchmark of the MI355X FNO3d path (contract: see the task statement / DESIGN.md).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--full]

N>1: either launched by ``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`` (WORLD_SIZE set: this
process is one rank) or started plainly as ``python bench.py --gpus N``: it then re-executes itself under
torch.distributed.run with N ranks on 127.0.0.1, one per GPU over RCCL, and the ranks' JSON line is this run's line.

One "step" = one full training iteration of the reference's hot loop (train.py:321-334: forward, MSE mean,
backward, Adam, cosine LR) on a synthetic batch of BASELINE.json configs[1]: FNO3d cylinder-shaped
[B=32/GPU, 20, 128, 128, 2], modes (4,12,16), width 64, 4 layers, fp32.  Inputs are resident in HBM when the
timed region starts.  Rank 0 prints ONE JSON line with the whole-job samples/s and the roofline of the dominant
kernel (HIP-event timed inside the timed region).  A plain run does nothing else: it sets up, warms up, times the K steps,
writes --dump-outputs and prints the line.  ``--full`` adds what takes runs of its own: the parity checks against the
reference fixtures, the rollout, the live PMC traffic and chip ceilings, the scaling proxy, the secondary models and
configurations, and a CPU baseline (the oracle timed on the host cores); the ``--no-*`` options leave parts of it out.
That line is the compact form of the result record (scalars and short labels); ``--record FILE`` writes the whole record.
``--dump-outputs DIR`` writes what the last timed step computed as ``DIR/<name>.npy`` (see ``dump_outputs``): the inputs are
seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s
MFMA_F32_PEAK_TF = 157.3     # fp32-input MFMA = fp32 vector peak
MFMA_BF16_PEAK_TF = 2500.0   # dense bf16 MFMA (MI355X_MICROARCH.md)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="trajectories per GPU (weak scaling) / in total (--scaling strong)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak (default, the headline): --batch trajectories on EVERY GPU; strong: --batch trajectories in total, "
                         "--batch / N per GPU (SURVEY.md section 8d/e asks for both)")
    ap.add_argument("--no-fno-native", action="store_true", help="skip the FNO3d line at the reference-native cylinder shape [32,20,64,128,3]")
    ap.add_argument("--rollout-steps", type=int, default=10, help="N_autoregressive of configs/cylinder/fno.yaml")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-rollout", action="store_true")
    ap.add_argument("--no-scaling-proxy", action="store_true", help="skip the one-rank strong-scaling proxy (step at B = 16 / 8 / 4 with the DP path on)")
    ap.add_argument("--profile-all", action="store_true", help="print per-kernel HIP-event table to stderr")
    ap.add_argument("--no-transolver", action="store_true", help="skip the secondary Transolver measurement")
    ap.add_argument("--no-galerkin", action="store_true", help="skip the secondary Galerkin Transformer measurement")
    ap.add_argument("--no-dpot", action="store_true", help="skip the secondary DPOT-S measurement")
    ap.add_argument("--no-unet", action="store_true", help="skip the secondary U-Net measurements (cylinder YAML and C3 mesh)")
    ap.add_argument("--no-bf16", action="store_true", help="skip the bf16-storage FNO rollout (BASELINE.json configs[4])")
    ap.add_argument("--no-pmc", action="store_true", help="take roofline.traffic from profiles/traffic_per_launch.json instead of measuring it "
                    "now (default at N=1: two rocprofv3 --pmc request-size passes over tools/kbench.py cell_mix, --kernel-trace only, ~40 s)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline figure: loss / gradient checks against the reference fixtures, rollouts, live PMC traffic, "
                         "copy / MFMA ceilings, N > 1 collective timing, scaling proxy, secondary models and CPU baseline (the --no-* "
                         "options and --only-headline select within it); without it a run only sets up, warms up, times the steps, "
                         "writes --dump-outputs and prints the line")
    ap.add_argument("--only-headline", action="store_true", help="with --full: the FNO train step only: no rollout, secondary models, PMC passes or CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (loss, updated parameters, parameter gradients; "
                         "large tensors as a fixed seeded sample) as DIR/<name>.npy, float32, <= 64 MB in all")
    ap.add_argument("--record", metavar="FILE", default=None,
                    help="write the full result record (every nested table and note) as JSON to FILE; stdout carries its compact form")
    ap.add_argument("--cpu-baseline-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--proxy-worker", type=float, default=None, help=argparse.SUPPRESS)     # child process of the scaling proxy: ms of the B = 32 step
    a = ap.parse_args(argv)
    if a.steps < 1:
        ap.error("--steps must be >= 1")
    if a.only_headline or not a.full:
        a.no_cpu_baseline = a.no_rollout = a.no_transolver = a.no_galerkin = a.no_dpot = a.no_unet = a.no_bf16 = a.no_pmc = True
        a.no_scaling_proxy = True
        a.no_fno_native = True
    return a


def self_launch(a):
    """``python bench.py --gpus N`` without a launcher: spawn the N ranks ourselves (one process per GPU, RCCL)."""
    import socket
    import subprocess
    n_vis = torch.cuda.device_count()
    share = os.environ.get("RPB_BENCH_SHARE_GPU") == "1"      # plumbing test on a 1-GPU box: ranks share cuda:0 over gloo
    if n_vis < a.gpus and not share:
        raise SystemExit(f"bench.py --gpus {a.gpus}: only {n_vis} GPU(s) visible on this node")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


DUMP_BUDGET_BYTES = 64 << 20
DUMP_MAX_ELEMS = 1 << 17          # per tensor; larger tensors are dumped as a seeded sample of this many entries


def dump_outputs(out_dir, loss, model, grad):
    """What the last timed ``Trainer.step`` hands its caller: the loss, and the model it updated -- parameters (reference-format
    state dict, BatchNorm running statistics included) and the parameter gradients of that step.  float32; complex tensors as
    (real, imag) pairs; a tensor over DUMP_MAX_ELEMS entries is dumped as the entries at sorted indices drawn without replacement by
    numpy's default_rng seeded with the CRC-32 of its name (the same for every run and build).  Returns {name: shape}.
    The training step is bit-reproducible, so two runs of one build match exactly.  Across builds compare with a tolerance, and
    expect the convs.*.bias gradients to be rounding noise: BatchNorm cancels them, and Adam turns that noise into full-size moves
    of those biases and of the BatchNorm running means."""
    import zlib
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss": loss.detach().float().reshape(-1)}
    for prefix, sd in (("param", model.state_dict()), ("grad", model.grads_as_state_dict(grad))):
        for k, v in sd.items():
            arrays[f"{prefix}.{k}"] = v
    total, shapes = 0, {}
    for name, t in arrays.items():
        t = t.detach()
        t = torch.view_as_real(t.resolve_conj()) if t.is_complex() else t
        a = t.float().cpu().numpy().reshape(-1)
        if a.size > DUMP_MAX_ELEMS:
            idx = np.random.default_rng(zlib.crc32(name.encode())).choice(a.size, DUMP_MAX_ELEMS, replace=False)
            a = a[np.sort(idx)]
        total += a.nbytes
        if total > DUMP_BUDGET_BYTES:
            raise SystemExit(f"bench.py --dump-outputs: {total} bytes exceed the {DUMP_BUDGET_BYTES}-byte budget at {name}")
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))
        shapes[name] = list(a.shape)
    return shapes


def _line_scalar(v):
    if isinstance(v, str):
        return len(v) <= 160
    if isinstance(v, list):
        return len(v) <= 16 and all(isinstance(e, (int, float)) and not isinstance(e, bool) for e in v)
    return v is None or isinstance(v, (bool, int, float))


def compact_line(line):
    """The stdout form of the result record: every top-level scalar, and of every top-level object its scalars, short strings and
    short numeric lists.  Deeper tables and long notes stay in the full record (--record); ``roofline`` keeps flat copies of its
    nested figures for this reason."""
    out = {}
    for k, v in line.items():
        if isinstance(v, dict):
            out[k] = {kk: vv for kk, vv in v.items() if _line_scalar(vv)}
        elif _line_scalar(v):
            out[k] = v
    return out


def usable_cores():
    """Host cores this process may really use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period))))
    except Exception:
        pass
    return n


def cpu_baseline_worker():
    """Child process: SURVEY.md section 8(d) / BASELINE.md section 3 -- the CPU oracle (PyTorch-CPU restatement of the
    reference, pinned to reference vectors) runs BASELINE.json configs[0] exactly: B=4, [20,128,128,2], modes (4,12,16),
    width 64, 4 layers; 1 warm-up + 3 timed train steps (zero_grad -> fwd -> MSE mean -> bwd -> Adam -> cosine), then a
    10-step autoregressive rollout.  One JSON line per finished part, so a timeout still leaves the train number."""
    from oracle import fno3d_oracle as O
    from realpdebench_amd.synthetic import normal_batch
    shape, modes, width, n_layers = (20, 128, 128, 2), (4, 12, 16), 64, 4
    cores = min(usable_cores(), 64)
    torch.set_num_threads(cores)
    Bc, nsteps = 4, 3
    sd = O.init_state_dict(modes, n_layers, width, shape, shape, seed=0)
    batches = [(normal_batch(10 + 2 * i, Bc, *shape), normal_batch(11 + 2 * i, Bc, *shape)) for i in range(nsteps + 1)]
    stamps = []
    O.train_steps(sd, batches, modes, n_layers, shape, shape, lr0=1e-4, t_max=4000, stamps=stamps)   # step 0 = warm-up
    times = [b - a for a, b in zip(stamps[:-1], stamps[1:])]
    res = {"value": Bc / (sum(times) / nsteps), "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
           "best_samples_per_s": Bc / min(times),
           "sample": f"BASELINE.json configs[0]: CPU oracle, B={Bc}, 1 warm-up + {nsteps} timed train steps "
                     f"(fwd+MSE+bwd+Adam+cosine), mean {sum(times) / nsteps:.1f} s/step, min {min(times):.1f} s"}
    print(json.dumps(res), flush=True)
    n_ar = 10
    with torch.no_grad():
        t0 = time.time()
        O.rollout(sd, batches[0][0], n_ar, modes, n_layers, shape, shape)
        rt = time.time() - t0
    res["rollout"] = {"value": Bc * shape[0] * n_ar / rt, "unit": "fields/s", "n_autoregressive": n_ar,
                      "sample": f"{n_ar}-step autoregressive rollout at B={Bc}, {rt:.1f} s"}
    print(json.dumps(res), flush=True)


def cpu_baseline(timeout=480):
    """Bounded: runs in a child process with a hard timeout so the default bench always finishes in minutes; whatever part
    of the sample finished before the timeout is reported."""
    import subprocess
    out = ""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker"], capture_output=True,
                           text=True, timeout=timeout)
        out = r.stdout
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    if lines:
        return json.loads(lines[-1])
    return {"value": None, "unit": "samples/s", "cores": usable_cores(), "kind": "port",
            "sample": f"CPU oracle sample (configs[0], B=4) did not finish one part within {timeout} s"}


PMC_REQUEST_BYTES = {"TCC_EA0_RDREQ_32B": 32, "TCC_EA0_RDREQ_64B": 64, "TCC_EA0_RDREQ_128B": 128, "TCC_EA0_WRREQ_64B": 64}


def pmc_bytes_per_dispatch(csv_path, kernel_substring):
    """{kernel name: mean over its dispatches of sum_counters request_size * count} from a rocprofv3 *_counter_collection.csv."""
    import csv
    acc = {}
    for r in csv.DictReader(open(csv_path)):
        if kernel_substring in r["Kernel_Name"] and r["Counter_Name"] in PMC_REQUEST_BYTES:
            k = (r["Kernel_Name"], r["Dispatch_Id"])
            acc[k] = acc.get(k, 0.0) + PMC_REQUEST_BYTES[r["Counter_Name"]] * float(r["Counter_Value"])
    per = {}
    for (kn, _), v in acc.items():
        per.setdefault(kn, []).append(v)
    return {kn: sum(v) / len(v) for kn, v in per.items()}


def cell_mix_family_bytes(per_kernel):
    """per_kernel: {kernel name: {"rd": bytes, "wr": bytes}} -> bytes per launch averaged over one train step's mix of the family:
    3 x forward + BatchNorm sums, 1 x layer 0 on the feature fields, 3 x backward + BatchNorm-backward sums."""
    tot = {kn: t["rd"] + t["wr"] for kn, t in per_kernel.items() if "rd" in t and "wr" in t}
    pick = lambda sub: next(v for k, v in tot.items() if sub in k)
    # template arguments <STATS, BF, FEAT, DFT, WG>; round 4: the backward launch of the step is the wave-pair variant (WG) that also
    # forms the Conv3d weight gradient (same algorithmic bytes as the plain STATS = 2 launch)
    # (prefix match: template parameters appended later -- H2 in round 6 -- must not break the lookup)
    return (3 * pick("<1, false, false, false, false, false, 0") + pick("<1, false, true, false, false, false, 0") + 3 * pick("<2, false, false, false, true, false, 0")) / 7


def live_pmc_traffic(family):
    """HBM bytes per launch of the cell_mix family from rocprofv3 request-size counters, collected as MI355X_MICROARCH.md prescribes:
    separate --pmc passes with --kernel-trace only (read: 32 / 64 / 128 B requests, write: 64 B requests; FETCH_SIZE under-reports
    128 B requests on gfx950), over tools/kbench.py at the bench's sizes (B = 32).  Family average over one step's launch mix
    (3 x fwd + BN sums, 1 x layer 0, 3 x bwd + BN-backward sums).  Returns (bytes, source) or (None, None)."""
    import glob
    import shutil
    import subprocess
    import tempfile
    if family != "cell_mix" or not shutil.which("rocprofv3"):
        return None, None
    passes = {"rd": "TCC_EA0_RDREQ_32B TCC_EA0_RDREQ_64B TCC_EA0_RDREQ_128B", "wr": "TCC_EA0_WRREQ_64B"}
    per_kernel = {}
    try:
        for tag, counters in passes.items():
            d = tempfile.mkdtemp(prefix=f"rpb_pmc_{tag}_", dir="/tmp")
            subprocess.run(["rocprofv3", "--pmc", *counters.split(), "--kernel-trace", "--output-format", "csv", "-d", d, "--",
                            sys.executable, os.path.join(ROOT, "tools", "kbench.py"), "cell_mix"], cwd="/tmp",
                           env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, timeout=90, check=True)
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            for kn, v in pmc_bytes_per_dispatch(files[0], "cmx_kernel").items():
                per_kernel.setdefault(kn, {})[tag] = v
            shutil.rmtree(d, ignore_errors=True)
        return cell_mix_family_bytes(per_kernel), ("live: rocprofv3 --pmc TCC_EA0_RDREQ_{32B,64B,128B} / TCC_EA0_WRREQ_64B passes over "
                                                   "tools/kbench.py cell_mix (this run)")
    except Exception as e:                              # no counters on this box / profiler refused: fall back to the committed passes
        print(f"[bench] --pmc failed ({type(e).__name__}: {e}); using profiles/traffic_per_launch.json", file=sys.stderr)
        return None, None


def _flush_c_stdio():
    """RCCL prints its version banner through C stdio, which is fully buffered on a pipe and would otherwise land AFTER
    the JSON line when the process exits; push it out first so the JSON line is the last line of stdout."""
    sys.stdout.flush()
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass


SPLIT_BF16_PEAK_TF = MFMA_BF16_PEAK_TF / 6.0      # one fp32-grade product = six bf16 MFMA products (csrc/rpb_conv3x.hip)
SPLIT_LABELS = ("conv3x", "gemm3x", "conv3x_wgrad", "gemm3x_tn")      # families on the split-bf16 matrix pipe (ops.py labels up to "[")


HBM_LABELS = ("axis_gemm", "axis_gemm_bf16in")


def pipe_rooflines(summary, steps):
    """Per-kernel MEASURED work of one profiled train step (HIP events around every launch; flops / algorithmic bytes are
    the per-launch figures ops.py attaches), grouped by the pipe that executes it: split-bf16 MFMA (fp32-grade convolutions and
    token GEMMs), fp32 MFMA, and HBM-bound kernels (no matrix work).  Fractions are against the pipe actually used."""
    pipes = {"split_bf16_mfma": [0.0, 0.0, 0.0], "f32_mfma": [0.0, 0.0, 0.0], "hbm": [0.0, 0.0, 0.0]}
    for label, v in summary.items():
        fam = label.split("[")[0]
        ai = v["flops"] / max(v["bytes"], 1.0)
        # the DFT stages run on the bf16 pipe at N % 64 == 0 but are HBM-bound by construction (K <= 268): booked against HBM
        pipe = "split_bf16_mfma" if fam in SPLIT_LABELS else ("f32_mfma" if ai > 8.0 and fam not in HBM_LABELS else "hbm")
        p = pipes[pipe]
        p[0] += v["total_ms"] / steps
        p[1] += v["flops"] * v["calls"] / steps
        p[2] += v["bytes"] * v["calls"] / steps
    tot = sum(p[0] for p in pipes.values())
    out = {"kernel_ms_per_step": tot}
    for name, (ms, fl, by) in pipes.items():
        if ms <= 0:
            continue
        e = {"ms_per_step": ms, "share_of_kernel_time": ms / tot}
        if name == "hbm":
            e.update(achieved=by / ms / 1e6, peak=HBM_PEAK_GBS, unit="GB/s", frac=by / ms / 1e6 / HBM_PEAK_GBS)
        else:
            peak = SPLIT_BF16_PEAK_TF if name == "split_bf16_mfma" else MFMA_F32_PEAK_TF
            e.update(achieved=fl / ms / 1e9, peak=peak, unit="TFLOP/s (fp32-equivalent)" if name == "split_bf16_mfma" else "TFLOP/s",
                     frac=fl / ms / 1e9 / peak, flops_per_step=fl)
        # a fraction above 1 means a family is booked on the wrong pipe (round 3: gemm3x_tn was missing from SPLIT_LABELS)
        assert e["frac"] <= 1.0, f"pipe_rooflines: {name} fraction {e['frac']:.3f} > 1 -- a kernel family is booked on the wrong pipe"
        out[name] = e
    return out


def bench_model(dev, make_model, x, y, lr, steps, config, exact_line=False, forward=True, clip=0.0):
    """Train step (the reference's loop body through realpdebench_amd.trainer.make_trainer) and eval forward of one of the
    secondary models; one extra step runs with HIP events around every launch for the measured per-pipe rooflines."""
    from realpdebench_amd import _lib, ops
    from realpdebench_amd.trainer import make_trainer
    torch.manual_seed(0)
    m = make_model().to(dev)
    tr = make_trainer(m, lr=lr, num_update=4000, clip_grad_norm=clip)
    B = x.shape[0]

    def timed(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            tr.step(x, y)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    timed(2)                                # two warm-up steps: the first one pays allocator growth and code loading
    t_train = timed(steps)
    _lib.PROFILE, _lib.PROFILE_ONLY = {}, None
    timed(1)
    prof = _lib.profile_summary()
    _lib.PROFILE = None
    if os.environ.get("RPB_BENCH_TABLE"):            # per-kernel HIP-event table of the profiled step (stderr)
        for label, v in sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"]):
            print(f"{label:44s} calls {v['calls']:4d}  total {v['total_ms']:8.3f} ms  {v['bytes'] * v['calls'] / v['total_ms'] / 1e6:8.1f} GB/s"
                  f"  {v['flops'] * v['calls'] / v['total_ms'] / 1e9:7.2f} TF/s", file=sys.stderr)
    res = {"train_samples_per_s": B / t_train, "ms_per_step": 1e3 * t_train, "batch": B,
           "trainer": type(tr).__name__, "roofline": pipe_rooflines(prof, 1),
           "peak_mem_GiB": torch.cuda.max_memory_allocated() / 2 ** 30, "config": config}
    if exact_line:                          # the same step with every convolution / GEMM on the exact-fp32 MFMA kernels
        ops.CONV3_SPLIT, ops.GEMM_SPLIT = False, False
        try:
            timed(1)
            res["exact_f32_ms_per_step"] = 1e3 * timed(steps)
        finally:
            ops.CONV3_SPLIT, ops.GEMM_SPLIT = True, True
    if forward:
        m.eval()
        with torch.no_grad():
            m(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                m(x)
            torch.cuda.synchronize()
        t_fwd = (time.perf_counter() - t0) / steps
        res.update(forward_fields_per_s=B * y.shape[1] / t_fwd, ms_per_forward=1e3 * t_fwd)
    del m, tr
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return res


def _yaml(*path):
    import yaml
    with open(os.path.join(ROOT, "realpdebench_amd", "configs", *path)) as fh:
        return yaml.safe_load(fh)


def bench_unet(dev, steps=2):
    """U-Net at the reference's configs/cylinder/unet.yaml ([12,20,64,128,3], dim = H = 64 -> 64/128/256 channels)."""
    from realpdebench_amd.model.unet import Unet3d
    cfg = _yaml("cylinder", "unet.yaml")
    T, H, W, C = cfg["shape_in"]
    B = int(cfg["train_batch_size"])
    x = torch.randn(B, T, H, W, C, device=dev)
    y = torch.randn(B, *cfg["shape_out"], device=dev)
    return bench_model(dev, lambda: Unet3d(dim=H, out_channels=cfg["shape_out"][-1], dim_mults=cfg["dim_mults"], channels=C,
                                           in_time=T, out_time=cfg["shape_out"][0]), x, y, cfg["lr"], steps,
                       "configs/cylinder/unet.yaml: [12,20,64,128,3], dim 64, dim_mults [1,2,4], 4 heads x 32",
                       exact_line=True)


def bench_unet_c3(dev, steps=1):
    """BASELINE.json configs[2]: U-Net on the fsi-shaped 20 x 256 x 256 sample, dim = H = 256 (load_model.py:52) -> 256/512/1024
    channels, at the configuration's 16 samples per GPU (B = 128 over 8 GPUs).  One fp32 sample peaks at ~116 GiB of activations, so
    the step runs as 16 micro-batches of one sample with accumulated gradients and ONE optimizer update (ArenaTrainer(micro_batch=1):
    the same step, exactly -- the model has no batch statistics).  First the one-sample step with its per-pipe rooflines, then one
    timed 16-sample step."""
    from realpdebench_amd.model.unet import Unet3d
    from realpdebench_amd.trainer import make_trainer
    make = lambda: Unet3d(dim=256, out_channels=3, dim_mults=[1, 2, 4], channels=3, in_time=20, out_time=20)
    x = torch.randn(1, 20, 256, 256, 3, device=dev)
    y = torch.randn(1, 20, 256, 256, 3, device=dev)
    r = bench_model(dev, make, x, y, 1e-4, steps, "U-Net fsi-shaped C3 mesh [1,20,256,256,3], dim 256 -> 256/512/1024 channels", forward=False)
    torch.manual_seed(0)
    m = make().to(dev)
    tr = make_trainer(m, lr=1e-4, num_update=4000, micro_batch=1)
    tr.step(x, y)                                    # warm-up at one sample (allocator, code loading)
    B = 16
    xb, yb = torch.randn(B, 20, 256, 256, 3, device=dev), torch.randn(B, 20, 256, 256, 3, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.step(xb, yb)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    r["per_gpu_batch_16"] = {"batch": B, "micro_batch": 1, "ms_per_step": 1e3 * dt, "train_samples_per_s": B / dt,
                             "peak_mem_GiB": torch.cuda.max_memory_allocated() / 2 ** 30}
    r["note"] = ("BASELINE configs[2] asks B=128 over 8 GPUs = 16 per GPU: run as 16 accumulated one-sample passes per optimizer step "
                 "(fp32 activations of one sample take ~116 GiB)")
    del m, tr
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return r


def bench_dpot(dev, steps=3):
    """DPOT-S at the reference's configs/cylinder/dpot_s.yaml ([16,20,128,128,2] -> 16 x 16 patches, embed 1024, depth 6)."""
    from realpdebench_amd.model.load_model import load_model
    cfg = _yaml("cylinder", "dpot_s.yaml")
    B = int(cfg["train_batch_size"])
    x = torch.randn(B, *cfg["shape_in"], device=dev)
    y = torch.randn(B, *cfg["shape_out"], device=dev)
    ds = [(x[0], y[0])]
    return bench_model(dev, lambda: load_model(ds, device="cpu", **cfg), x, y, cfg["lr"], steps,
                       "configs/cylinder/dpot_s.yaml: [16,20,128,128,2], patch 8, embed 1024 in 8 blocks, depth 6, 20 -> 20 frames, "
                       "random initial weights", clip=float(cfg["clip_grad_norm"]))


def bench_galerkin(dev, steps=3):
    """Galerkin Transformer at the reference's configs/cylinder/galerkin_transformer.yaml (n = 20*64*128 tokens, hidden 256,
    freq_dim 128, modes (4,16,20), train_batch_size 16)."""
    from realpdebench_amd.model.galerkin_transformer import GalerkinTransformer3d
    cfg = _yaml("cylinder", "galerkin_transformer.yaml")
    T, H, W, Cin = cfg["shape_in"]
    B = int(cfg["train_batch_size"])
    cfg.update(node_feats=Cin, n_targets=cfg["shape_out"][-1])
    x = torch.randn(B, T, H, W, Cin, device=dev)
    y = torch.randn(B, *cfg["shape_out"], device=dev)
    return bench_model(dev, lambda: GalerkinTransformer3d(**cfg), x, y, cfg["lr"], steps,
                       "configs/cylinder/galerkin_transformer.yaml: [16,20,64,128,3], n_hidden 256, 4 heads, freq_dim 128, "
                       "modes (4,16,20), dropout 0.05 / attention 0.5")


def bench_transolver(dev, B=4, steps=3):
    """Transolver (configs/cylinder/trainsolver.yaml: 20x64x128x3 tokens -> mesh 128x64x20, hidden 256, 8 heads, 16
    slices, 1 layer, dropout 0.1)."""
    from realpdebench_amd.model.transolver import Transolver
    x = torch.randn(B, 20, 64, 128, 3, device=dev)
    y = torch.randn(B, 20, 64, 128, 3, device=dev)
    return bench_model(dev, lambda: Transolver(space_dim=3, n_layers=1, n_hidden=256, n_head=8, fun_dim=0, out_dim=3,
                                               slice_num=16, mlp_ratio=4, H=128, W=64, D=20, dropout=0.1), x, y, 7e-4, steps,
                       "Transolver cylinder: tokens 20x64x128 -> mesh (128,64,20), n_hidden 256, 8 heads, 16 slices, "
                       "1 layer, mlp_ratio 4, dropout 0.1, fp32", exact_line=True)


def bench_transolver_b16(dev):
    """The same model at the reference YAML's train_batch_size (configs/cylinder/trainsolver.yaml: 16)."""
    r = bench_transolver(dev, B=16, steps=2)
    r.pop("exact_f32_ms_per_step", None)
    return r


def bench_transolver_c4(dev, B=8, steps=3):
    """BASELINE.json configs[3]: Transolver at the foil-shaped 64 x 64 sample [B,20,64,64,3] -> mesh (64,64,20) (the H / W / D of the
    reference's 64 x 64 trainsolver YAMLs), hidden 256, 8 heads, 16 slices, 1 layer, dropout 0.1; 81 920 tokens per sample."""
    from realpdebench_amd.model.transolver import Transolver
    x = torch.randn(B, 20, 64, 64, 3, device=dev)
    y = torch.randn(B, 20, 64, 64, 3, device=dev)
    r = bench_model(dev, lambda: Transolver(space_dim=3, n_layers=1, n_hidden=256, n_head=8, fun_dim=0, out_dim=3,
                                            slice_num=16, mlp_ratio=4, H=64, W=64, D=20, dropout=0.1), x, y, 7e-4, steps,
                    "Transolver C4 (foil-shaped): tokens 20x64x64 -> mesh (64,64,20), n_hidden 256, 8 heads, 16 slices, 1 layer, "
                    "mlp_ratio 4, dropout 0.1, fp32 storage")
    r["ms_per_sample"] = r["ms_per_step"] / B
    # 25.7 MFLOP per token and step, 81 920 tokens per sample, against the fp32 matrix pipe (the north star's
    # roofline for this model) and against the split-bf16 pipe the convolutions and token GEMMs actually run on
    fl = 25.7e6 * 81920 * B
    r["flop_model"] = {"flops_per_step": fl, "achieved_TFLOPs": fl / r["ms_per_step"] / 1e9,
                       "x_f32_mfma_roofline_of_survey_8d": fl / r["ms_per_step"] / 1e9 / MFMA_F32_PEAK_TF,   # a RATIO (> 1 allowed): the kernels run on the bf16 pipe
                       "frac_of_split_bf16_peak": fl / r["ms_per_step"] / 1e9 / SPLIT_BF16_PEAK_TF}
    return r


def bench_rollout_bf16(dev):
    """BASELINE.json configs[4]: FNO3d on the 64^3 combustion volume, bf16 activation storage, 20 autoregressive steps."""
    try:
        from realpdebench_amd.model.fno import FNO3d
        if not hasattr(FNO3d, "set_storage"):
            return {"status": "not built"}
    except Exception as e:                                      # pragma: no cover
        return {"status": f"unavailable: {e}"}
    from realpdebench_amd.rollout import autoregressive_rollout
    shape, modes, L, B, n_ar = (64, 64, 64, 16), (4, 16, 16), 4, 16, 20
    torch.manual_seed(0)
    m = FNO3d(*modes, L, 64, shape, shape).to(dev).eval()
    x = torch.randn(B, *shape, device=dev)
    res = {}
    outs = {}
    for storage in ("f32", "bf16"):
        m.set_storage(storage)
        autoregressive_rollout(m, x, n_ar)                      # warm-up at full length: the 21 GB result block is then in the allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs[storage] = autoregressive_rollout(m, x, n_ar)
        torch.cuda.synchronize()
        rt = time.perf_counter() - t0
        bpe = 2 if storage == "bf16" else 4
        fwd_bytes = (0.445 * bpe / 2 * B + 0.537) * 1e9       # 2 B/element activations, fp32 weights
        res[storage] = {"value": B * shape[0] * n_ar / rt, "unit": "fields/s", "ms_per_forward": 1e3 * rt / n_ar,
                        "roofline": {"bound": "hbm", "algorithmic_bytes_per_forward": fwd_bytes,
                                     "achieved": fwd_bytes / (1e9 * rt / n_ar), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                     "frac": fwd_bytes / (1e9 * rt / n_ar) / HBM_PEAK_GBS}}
    d = (outs["bf16"].float() - outs["f32"]).double()
    T = shape[0]
    res["tolerance"] = "stated by this repo (the reference has no bf16 path): Rel-L2 vs the fp32 path < 2e-3 after 1 step, < 1e-2 after 20"
    res["rel_l2_vs_f32_step1"] = float(d[:, :T].norm() / outs["f32"][:, :T].double().norm())
    res["rel_l2_vs_f32_step20"] = float(d[:, -T:].norm() / outs["f32"][:, -T:].double().norm())
    res["config"] = f"FNO3d combustion volume [B={B},64,64,64,16] -> padded 70^3, modes (4,16,16), width 64, 4 layers, {n_ar} AR steps"
    from realpdebench_amd import _lib
    res["bf16_const_planes"] = _lib.query("rpb_bf16_const_planes")      # compile-time switch of the library (round-5 advisor finding: say it)
    res["bf16_const_planes_note"] = ("planes of the fp32 constants multiplied with bf16-STORED operands (library build switch; 3 until round 4, "
                                     "2 since round 5 with the end-to-end rel_l2_vs_f32_step1 measured unchanged at 3.3e-4); the rel_l2 "
                                     "values of this object are THIS build's end-to-end rollout errors")
    m.set_storage("f32")
    del m
    torch.cuda.empty_cache()
    return res


def fno_step_bytes(B, T, H, W, Cin, Cout_r, width, L, modes, pad=6):
    """algorithmic bytes of one FNO3d train step and of one eval forward."""
    Tp, Hp, Wp = T + pad, H + pad, W + pad
    n_in, n_out = B * T * H * W * Cin, B * T * H * W * Cout_r
    n_u, n_p = B * width * T * H * W, B * width * Tp * Hp * Wp
    M = 4 * modes[0] * modes[1] * modes[2]
    wspec = width * width * M * 8
    p_real = L * (2 * width * width * M + width * width + 3 * width) + width * (Cin + 3) + width + 128 * width + 128 + Cout_r * 128 + Cout_r
    step = 4 * ((12 * L + 2) * n_p + 3 * n_u + n_in + 3 * n_out) + 3 * L * wspec + 28 * p_real
    fwd = 4 * (n_in + n_out + (2 * L + 1) * n_p + n_u) + L * wspec
    return float(step), float(fwd)


def copy_ceiling(dev, n=14939392 * 64):
    """The streaming ceiling of THIS chip for the read / write mixes of the FNO kernels, measured now with the library's plain
    streaming kernel (csrc/rpb_probe.hip) on buffers of one activation tensor's size (3.82 GB): GB/s for 1, 2 and 3 tensors read + one
    written.  A kernel that moves its algorithmic bytes exactly once cannot beat this rate, whatever the 8 TB/s datasheet says."""
    from realpdebench_amd import ops
    bufs = [torch.zeros(n, device=dev) for _ in range(4)]
    res = {}
    for nr in (1, 2, 3):
        best = 0.0
        for threads in (256, 512):
            ops.stream_probe(bufs[0], bufs[1], bufs[2], bufs[3], nr, threads)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                ops.stream_probe(bufs[0], bufs[1], bufs[2], bufs[3], nr, threads)
            e1.record()
            torch.cuda.synchronize()
            best = max(best, 5 * 4.0 * n * (nr + 1) / (e0.elapsed_time(e1) * 1e6))
        res[f"r{nr}w1"] = best
    del bufs
    torch.cuda.empty_cache()
    return res


def _num_cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def mfma_ceiling(dev):
    """Sustained bf16 MFMA rate of THIS chip (csrc/rpb_probe.hip: 4 independent 32x32x16 chains per wave, one wave per SIMD, register
    operands) with random operands -- the power-limited rate real data sees -- and with zeros (the datasheet-like rate).  TFLOP/s."""
    from realpdebench_amd import ops
    res = {}
    out = torch.empty(256 * 2 * 512, device=dev)
    for name, seed in (("random_operands", torch.randn(4096, device=dev)), ("zero_operands", torch.zeros(4096, device=dev))):
        ops.mfma_probe(seed, out, 2000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fl = ops.mfma_probe(seed, out, 40000)
        e1.record()
        torch.cuda.synchronize()
        res[name] = fl / (e0.elapsed_time(e1) * 1e9)
    return res


def bench_fno_native(dev, steps=5, shape=(20, 64, 128, 3), modes=(4, 12, 16), width=64, L=4, B=32, config=None):
    """FNO3d at the reference-native cylinder sample shape (realpdebench/configs/cylinder/fno.yaml with the released data:
    [32,20,64,128,3] -> padded 26 x 70 x 134), same modes / width / depth: fused Trainer.step and the 10-step rollout."""
    from realpdebench_amd.model.fno import FNO3d
    from realpdebench_amd.rollout import autoregressive_rollout
    from realpdebench_amd.trainer import Trainer
    torch.manual_seed(0)
    m = FNO3d(*modes, L, width, shape, shape).to(dev)
    tr = Trainer(m, lr=1e-4, num_update=4000)
    x, y = torch.randn(B, *shape, device=dev), torch.randn(B, *shape, device=dev)
    for _ in range(2):
        tr.step(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(x, y)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    step_b, fwd_b = fno_step_bytes(B, *shape, shape[-1], width, L, modes)
    res = {"train_samples_per_s": B / dt, "ms_per_step": 1e3 * dt, "batch": B,
           "roofline": {"bound": "hbm", "algorithmic_bytes": step_b, "achieved": step_b / dt / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": step_b / dt / 1e9 / HBM_PEAK_GBS},
           "peak_mem_GiB": torch.cuda.max_memory_allocated() / 2 ** 30,
           "config": config or "FNO3d [32,20,64,128,3] -> padded 26x70x134, modes (4,12,16), width 64, 4 layers (the reference's cylinder sample shape)"}
    del tr
    m._ws = {}
    torch.cuda.empty_cache()
    n_ar = 10
    autoregressive_rollout(m, x, n_ar)
    rts = []
    for _ in range(3):                  # three full rollouts, the line carries their mean (a single one was seen 20 % off inside the long bench process)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        autoregressive_rollout(m, x, n_ar)
        torch.cuda.synchronize()
        rts.append((time.perf_counter() - t0) / n_ar)
    rt = sum(rts) / len(rts)
    res["rollout"] = {"value": B * shape[0] / rt, "unit": "fields/s", "ms_per_forward": 1e3 * rt, "n_autoregressive": n_ar,
                      "runs": len(rts), "ms_per_forward_min": 1e3 * min(rts), "ms_per_forward_max": 1e3 * max(rts),
                      "roofline": {"bound": "hbm", "algorithmic_bytes_per_forward": fwd_b, "achieved": fwd_b / rt / 1e9,
                                   "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": fwd_b / rt / 1e9 / HBM_PEAK_GBS}}
    del m
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return res


def bench_fno_fsi(dev, steps=3):
    """FNO3d of the reference's configs/fsi/fno.yaml: width 128, modes (4,16,16), four layers, train_batch_size 32, on the fsi sample
    shape [20,64,64,3] -> padded 26 x 70 x 70 (spectral weights 4 x 537 MB)."""
    cfg = _yaml("fsi", "fno.yaml")
    shape = tuple(cfg["shape_in"])
    modes = (cfg["modes1"], cfg["modes2"], cfg["modes3"])
    return bench_fno_native(dev, steps=steps, shape=shape, modes=modes, width=cfg["width"], L=cfg["n_layers"], B=int(cfg["train_batch_size"]),
                            config=f"configs/fsi/fno.yaml: FNO3d [{cfg['train_batch_size']},{','.join(map(str, shape))}] -> padded 26x70x70, "
                                   f"modes {modes}, width {cfg['width']}, {cfg['n_layers']} layers")


def strong_scaling_proxy(dev, ms32, steps=5):
    """What one GPU can say about the 8-GPU strong-scaling run (fixed global batch 32): the step at the per-rank batches 16 / 8 / 4 with
    the WHOLE data-parallel path on (a one-rank RCCL process group: DataParallel, per-layer buckets through rpb_dp_* on the side
    stream, SyncBN reductions inline) -- step(32) / step(32 / N) is the ceiling of the N-rank speed-up whatever the interconnect does
    (batch-independent weight + Adam traffic, ~100 launches per step).  Kernel time of the B = 4 step next to its wall time says
    whether the small step is launch-bound."""
    import torch.distributed as dist
    from realpdebench_amd import _lib
    from realpdebench_amd.dp import DataParallel
    from realpdebench_amd.model.fno import FNO3d
    from realpdebench_amd.trainer import Trainer
    own_group = not dist.is_initialized()
    if own_group:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    shape, modes, width, L = (20, 128, 128, 2), (4, 12, 16), 64, 4
    res = {"how": "one-rank RCCL group, DataParallel + Trainer.step with the SyncBN reductions forced on (4 forward + 3 backward, inline on the "
                  "compute stream), 2 warm-up + %d timed steps per batch size" % steps,
           "ms_per_step": {"32": ms32}, "note_32": "B = 32: the headline line itself (no DP wrapper; RPB_FORCE_DP=1 measured equal)"}
    try:
        torch.manual_seed(0)
        model = FNO3d(*modes, L, width, shape, shape).to(dev)
        DataParallel(model)
        model.dp.sync_stats_always = True       # the 7 SyncBN reductions of an N-rank step run inline on the one-rank group as well
        tr = Trainer(model, lr=1e-4, num_update=4000)
        for B in (16, 8, 4):
            x, y = torch.randn(B, *shape, device=dev), torch.randn(B, *shape, device=dev)
            for _ in range(2):
                tr.step(x, y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(x, y)
            torch.cuda.synchronize()
            res["ms_per_step"][str(B)] = 1e3 * (time.perf_counter() - t0) / steps
            if B == 4:
                _lib.PROFILE, _lib.PROFILE_ONLY = {}, None
                tr.step(x, y)
                torch.cuda.synchronize()
                prof = _lib.profile_summary()
                _lib.PROFILE = None
                res["B4_kernel_ms"] = sum(v["total_ms"] for v in prof.values())
                res["B4_launches"] = sum(v["calls"] for v in prof.values())
                comm = getattr(model.dp, "comm", None)
                if comm is not None:
                    comm.set_timing(True)
                    tr.step(x, y)
                    torch.cuda.synchronize()
                    tms = comm.step_times()
                    res["B4_dp"] = {"exposed_comm_ms": tms["exposed_ms"], "buckets": len(tms["buckets"]),
                                    "syncbn_inline_reductions": len(tms["inline_ms"]), "syncbn_inline_ms_total": sum(tms["inline_ms"]),
                                    "syncbn_inline_ms_max": max(tms["inline_ms"] or [0.0])}
                    comm.set_timing(False)
            model._ws = {}
            del x, y
            torch.cuda.empty_cache()
        m = res["ms_per_step"]
        res["speedup_ceiling"] = {"2_ranks": ms32 / m["16"], "4_ranks": ms32 / m["8"], "8_ranks": ms32 / m["4"]}
        # ---- the 8-rank step's shape on ONE GPU (B = 4): the sharded optimizer step with pieces sized for 8 ranks (this rank updates 1/8 of
        # the arena: rpb_adam_step_ranges), and every collective idling its stream for the modelled ring transfer over 8 ranks
        # (rpb_dp_set_model: bus rate RPB_PROXY_GBPS, default 200 GB/s -- what RCCL reaches on 16 MB messages over 7 xGMI links is an
        # ESTIMATE until a node measures it -- plus RPB_PROXY_LAT_US = 15 us per phase), so that exposed communication shows up as time
        tr.close()
        del tr, model
        torch.cuda.empty_cache()
        gbps, lat = float(os.environ.get("RPB_PROXY_GBPS", "200")), float(os.environ.get("RPB_PROXY_LAT_US", "15"))
        x, y = torch.randn(4, *shape, device=dev), torch.randn(4, *shape, device=dev)
        variants = {}
        for name, shard, modelled in (("allreduce_modelled_comm", False, True), ("sharded_adam", True, False),
                                      ("sharded_adam_modelled_comm", True, True)):
            torch.manual_seed(0)
            model = FNO3d(*modes, L, width, shape, shape).to(dev)
            DataParallel(model, shard_optimizer=shard, shard_world=8 if shard else None)
            model.dp.sync_stats_always = True
            comm = getattr(model.dp, "comm", None)
            if modelled and comm is not None:
                comm.set_model(8, gbps, lat)
            tr = Trainer(model, lr=1e-4, num_update=4000)
            for _ in range(2):
                tr.step(x, y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(x, y)
            torch.cuda.synchronize()
            v = {"ms_per_step": 1e3 * (time.perf_counter() - t0) / steps}
            if comm is not None:
                comm.set_timing(True)
                tr.step(x, y)
                tr.step(x, y)        # (the second step's forward is what waits for the first one's parameter gathers)
                torch.cuda.synchronize()
                tms = comm.step_times()
                v.update(exposed_comm_ms=tms["exposed_ms"], collectives=len(tms["buckets"]),
                         modelled_comm_ms=sum(b["ms"] for b in tms["buckets"]), syncbn_inline_ms_max=max(tms["inline_ms"] or [0.0]),
                         gather_exposed_ms=tms.get("gather_exposed_ms"))
                comm.set_timing(False)
            v["speedup_ceiling_8_ranks"] = ms32 / v["ms_per_step"]
            variants[name] = v
            tr.close()
            del tr, model
            torch.cuda.empty_cache()
        res["B4_8rank_shape"] = {"model": {"ranks": 8, "bus_GBps": gbps, "latency_us_per_phase": lat,
                                           "note": "ring reduce-scatter / all-gather: bytes * 7/8 / rate + latency per phase; an all-reduce is two phases"},
                                 "variants": variants}
        res["speedup_ceiling"]["8_ranks_sharded_adam"] = variants["sharded_adam"]["speedup_ceiling_8_ranks"]
        res["speedup_ceiling"]["8_ranks_sharded_adam_modelled_comm"] = variants["sharded_adam_modelled_comm"]["speedup_ceiling_8_ranks"]
        tr = model = None
        res["byte_model_ceiling_8_ranks"] = (6.238 * 32 + 4.03) / (6.238 * 4 + 4.03)
        # ---- WEAK scaling (the mode the headline line declares: B = 32 per rank): the same one-GPU model of the 8-rank step at the full
        # per-rank batch, every collective idling its stream for the modelled ring transfer at the assumed and at a pessimistic bus rate;
        # efficiency = step(32, no DP) / step(32, 8-rank shape) -- what SCALE_rNN's 8-GPU point divided by 8x the 1-GPU point would show if
        # the interconnect delivered that rate
        del x, y
        torch.cuda.empty_cache()
        x, y = torch.randn(32, *shape, device=dev), torch.randn(32, *shape, device=dev)
        weak = {}
        for rate in (gbps, 0.5 * gbps):
            for name, shard in (("allreduce", False), ("sharded_adam", True)):
                torch.manual_seed(0)
                model = FNO3d(*modes, L, width, shape, shape).to(dev)
                DataParallel(model, shard_optimizer=shard, shard_world=8 if shard else None)
                model.dp.sync_stats_always = True
                comm = getattr(model.dp, "comm", None)
                if comm is not None:
                    comm.set_model(8, rate, lat)
                tr = Trainer(model, lr=1e-4, num_update=4000)
                for _ in range(2):
                    tr.step(x, y)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    tr.step(x, y)
                torch.cuda.synchronize()
                v = {"ms_per_step": 1e3 * (time.perf_counter() - t0) / steps}
                if comm is not None:
                    comm.set_timing(True)
                    tr.step(x, y)
                    tr.step(x, y)
                    torch.cuda.synchronize()
                    tms = comm.step_times()
                    v.update(exposed_comm_ms=tms["exposed_ms"], modelled_comm_ms=sum(b["ms"] for b in tms["buckets"]),
                             gather_exposed_ms=tms.get("gather_exposed_ms"))
                    comm.set_timing(False)
                v["efficiency_8_ranks"] = ms32 / v["ms_per_step"]
                weak[f"{name}_{int(rate)}GBps"] = v
                tr.close()
                del tr, model
                torch.cuda.empty_cache()
        tr = model = None
        res["weak_scaling_B32_8rank_shape"] = {"model": {"ranks": 8, "bus_GBps": [gbps, 0.5 * gbps], "latency_us_per_phase": lat}, "variants": weak}
        res["weak_scaling_modelled_efficiency_8"] = weak[f"allreduce_{int(gbps)}GBps"]["efficiency_8_ranks"]
        res["weak_scaling_modelled_efficiency_8_pessimistic"] = weak[f"allreduce_{int(0.5 * gbps)}GBps"]["efficiency_8_ranks"]
    finally:
        if own_group:
            dist.destroy_process_group()
        torch.cuda.empty_cache()
    return res


def family(label):
    return label.split("[")[0]


def by_family(summary):
    """HIP-event summary per label -> per kernel family (label up to '['): launches, total time, total algorithmic bytes /
    flops, and the variants it is made of."""
    fam = {}
    for label, v in summary.items():
        f = fam.setdefault(family(label), {"calls": 0, "total_ms": 0.0, "bytes": 0.0, "flops": 0.0, "variants": {}})
        f["calls"] += v["calls"]
        f["total_ms"] += v["total_ms"]
        f["bytes"] += v["bytes"] * v["calls"]
        f["flops"] += v["flops"] * v["calls"]
        f["variants"][label] = {"launches": v["calls"], "avg_launch_ms": v["avg_ms"],
                                "algorithmic_bytes_per_launch": v["bytes"],
                                "achieved_GBps": v["bytes"] / v["avg_ms"] / 1e6 if v["avg_ms"] else None,
                                "frac_of_hbm_peak": v["bytes"] / v["avg_ms"] / 1e6 / HBM_PEAK_GBS if v["avg_ms"] else None}
    return fam


def main():
    a = parse()
    if a.cpu_baseline_worker:
        return cpu_baseline_worker()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback path exists)")
    if a.proxy_worker is not None:
        torch.cuda.set_device(0)
        res = strong_scaling_proxy(torch.device("cuda", 0), float(a.proxy_worker))
        sys.stdout.flush()
        _flush_c_stdio()
        print("PROXY_JSON " + json.dumps(res), flush=True)
        return
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(a)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus and rank == 0:
        print(f"bench.py: --gpus {a.gpus} but the launcher started {world} rank(s); reporting n_gpus={world}", file=sys.stderr)
    share = os.environ.get("RPB_BENCH_SHARE_GPU") == "1"
    if share:
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    force_dp = os.environ.get("RPB_FORCE_DP") == "1"       # exercise the RCCL code path on a single rank
    backend = None
    if world > 1 or force_dp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        backend = "gloo" if share else "nccl"              # "nccl" IS RCCL on ROCm; gloo only for the shared-GPU plumbing test
        if share:
            dist.init_process_group(backend)
        else:
            dist.init_process_group(backend, device_id=dev)

    from realpdebench_amd import _lib
    from realpdebench_amd.model.fno import FNO3d
    from realpdebench_amd.rollout import autoregressive_rollout
    from realpdebench_amd.synthetic import bench_batch
    from realpdebench_amd.trainer import Trainer

    shape, modes, width, L = (20, 128, 128, 2), (4, 12, 16), 64, 4
    torch.manual_seed(0)
    model = FNO3d(*modes, L, width, shape, shape).to(dev)
    if world > 1 or force_dp:
        from realpdebench_amd.dp import DataParallel
        DataParallel(model)
    trainer = Trainer(model, lr=1e-4, num_update=4000, scheduler="cosine")
    if a.scaling == "strong":
        if a.batch % world:
            raise SystemExit(f"bench.py --scaling strong: --batch {a.batch} is not divisible by {world} ranks")
        B = a.batch // world                             # fixed GLOBAL batch: every rank takes its share
    else:
        B = a.batch
    if a.scaling == "strong" and world > 1:
        # the SAME global batch as the single-rank run of --batch (seeds of rank 0), cut into per-rank slices: with SyncBN and the
        # 1/N_global loss scale the N-rank step IS the 1-rank step on that batch (tests/test_gpu_dp.py checks the bench line for it)
        x, y = (t[rank * B:(rank + 1) * B].contiguous().to(dev) for t in bench_batch(a.batch, rank=0, shape=shape))
    else:
        x, y = (t.to(dev) for t in bench_batch(B, rank=rank, shape=shape))     # seeded N(0,1), identical on every host

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- warm-up with every launch timed: find the dominant kernel FAMILY (all template variants of one kernel)
    _lib.PROFILE, _lib.PROFILE_ONLY = {}, None
    first_loss = None
    for i in range(max(a.warmup, 1)):
        l_ = trainer.step(x, y)
        if i == 0:
            first_loss = float(l_)
    torch.cuda.synchronize()
    first_loss_global = first_loss
    if world > 1:                                        # mean over ranks of the local means = the global batch's loss
        t = torch.tensor([first_loss], device=dev, dtype=torch.float64)
        dist.all_reduce(t)
        first_loss_global = float(t) / world
    warm = _lib.profile_summary()
    fam_warm = by_family(warm)
    # (families that move no counted bytes -- partial reductions, finalize kernels -- can top a one-step warm-up of a tiny batch through
    #  their first-call overhead; the roofline is quoted on a family that has bytes)
    dominant = max((k for k in fam_warm if fam_warm[k]["bytes"] > 0), key=lambda k: fam_warm[k]["total_ms"])
    dom_labels = set(fam_warm[dominant]["variants"])
    if a.profile_all and rank == 0:
        tot = sum(v["total_ms"] for v in warm.values())
        for k, v in sorted(warm.items(), key=lambda kv: -kv[1]["total_ms"]):
            print(f"{k:48s} calls/step {v['calls'] / max(a.warmup, 1):5.1f}  avg {v['avg_ms']:8.3f} ms  "
                  f"{100 * v['total_ms'] / tot:5.1f}%  {v['bytes'] / v['avg_ms'] / 1e6:8.1f} GB/s  "
                  f"{v['flops'] / v['avg_ms'] / 1e9:7.2f} TF/s", file=sys.stderr)
        for k, v in sorted(fam_warm.items(), key=lambda kv: -kv[1]["total_ms"]):
            print(f"family {k:40s} {100 * v['total_ms'] / tot:5.1f}%  {v['total_ms'] / max(a.warmup, 1):7.2f} ms/step  "
                  f"{v['bytes'] / v['total_ms'] / 1e6:8.1f} GB/s", file=sys.stderr)

    # ---- parity guard on the timed workload itself (--full): the first-step loss of this exact batch / these exact weights must be
    #      the one the IMPORTED reference computed for them (tests/golden/make_golden_headline.py)
    loss_check = None
    if a.full and world == 1 and B == 32 and rank == 0:
        import numpy as np
        gz = np.load(os.path.join(ROOT, "tests", "golden", "fno3d_headline.npz"))
        ref = float(gz["b32/loss"])
        rel = abs(first_loss - ref) / abs(ref)
        loss_check = {"first_step_loss": first_loss, "reference_loss": ref, "rel_err": rel, "tol": 1e-5,
                      "source": "tests/golden/fno3d_headline.npz (imported reference, B=32, same seeds)"}
        if not rel < 1e-5:
            raise SystemExit(f"bench.py: first-step loss {first_loss!r} differs from the reference's {ref!r} (rel {rel:.2e}) "
                             "-- the timed path is not computing the reference's step; refusing to report a number")

    # ---- timed region: exactly K steps, only the dominant family's launches carry HIP events
    _lib.PROFILE, _lib.PROFILE_ONLY = {}, dom_labels
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = trainer.step(x, y)
    barrier()
    dt = time.perf_counter() - t0
    dom = by_family(_lib.profile_summary())[dominant]
    _lib.PROFILE = None
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    ms_per_step = 1e3 * dt / a.steps
    value = B * world * a.steps / dt

    # ---- --dump-outputs: the last timed step's results, before anything below steps the trainer again
    dumped = None
    if a.dump_outputs and rank == 0:
        dumped = {"dir": a.dump_outputs, "arrays": len(dump_outputs(a.dump_outputs, loss, model, trainer.grad))}

    # ---- N > 1: one more step with the collective instrumented (per-bucket schedule on the side stream, how long Adam waited for the
    #      last bucket, cost of the inline SyncBN reductions) -- outside the timed region, with --full (a plain run describes the setup only)
    dp_info = None
    if (world > 1 or force_dp) and model.dp is not None:
        comm = getattr(model.dp, "comm", None)
        dp_info = {"ranks_in_process_group": dist.get_world_size(), "backend": backend,
                   "transport": (f"C-ABI rpb_dp_* (RCCL, side HIP stream, {'two communicators' if comm.small != comm.handle else 'one communicator'})"
                                 if comm is not None else f"torch.distributed {backend}"),
                   "buckets_MB": [4e-6 * (e - s_) for s_, e in model.dp.buckets],
                   "optimizer_exchange": ("peer pointers: rpb_dp_p2p_* (no bucket travels; slice-owned reduce + Adam + broadcast)"
                                          if getattr(model.dp, "p2p_opt", False) else
                                          ("reduce-scatter + Adam on owned ranges + all-gather" if getattr(model.dp, "shard_opt", False)
                                           else "all-reduce buckets + full-arena Adam"))}
        if comm is not None and a.full:
            comm.set_timing(True)
            trainer.step(x, y)
            torch.cuda.synchronize()
            try:
                tms = comm.step_times()
                dp_info.update(exposed_comm_ms=tms["exposed_ms"], first_announce_to_last_done_ms=tms["first_announce_to_last_done_ms"],
                               bucket_schedule=tms["buckets"], syncbn_inline_reductions=len(tms["inline_ms"]),
                               syncbn_inline_ms_total=sum(tms["inline_ms"]), syncbn_inline_ms_max=max(tms["inline_ms"] or [0.0]))
            except Exception as e:                          # instrumentation must never cost the bench line
                dp_info["timing_error"] = repr(e)
            comm.set_timing(False)

    # ---- the chip's streaming ceiling for the kernels' read / write mixes, measured now (rank 0, --full)
    ceiling = mfma_peak = None
    if a.full and rank == 0:
        try:
            free_b = torch.cuda.mem_get_info()[0]
            if free_b > 20e9:
                ceiling = copy_ceiling(dev)
            mfma_peak = mfma_ceiling(dev)
        except Exception as e:
            print(f"[bench] copy-ceiling probe failed: {e!r}", file=sys.stderr)

    # ---- rollout metric (eval.py:311-321), replicas: no collective
    rollout = None
    if not a.no_rollout:
        del trainer
        model._ws = {}
        torch.cuda.empty_cache()
        autoregressive_rollout(model, x, a.rollout_steps)      # warm-up at full length (kernels compiled, result block cached)
        rts = []
        for _ in range(3):                                     # three full rollouts: the line carries their mean, min and max
            barrier()
            t0 = time.perf_counter()
            autoregressive_rollout(model, x, a.rollout_steps)
            barrier()
            rt1 = time.perf_counter() - t0
            if world > 1:
                t = torch.tensor([rt1], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                rt1 = float(t)
            rts.append(rt1)
        rt = sum(rts) / len(rts)
        fwd_bytes = (1.165 * B + 0.403) * 1e9            # algorithmic bytes of one eval forward
        rollout = {"value": B * world * shape[0] * a.rollout_steps / rt, "unit": "fields/s",
                   "n_autoregressive": a.rollout_steps, "ms_per_forward": 1e3 * rt / a.rollout_steps,
                   "runs": len(rts), "ms_per_forward_min": 1e3 * min(rts) / a.rollout_steps,
                   "ms_per_forward_max": 1e3 * max(rts) / a.rollout_steps,
                   "roofline": {"bound": "hbm", "algorithmic_bytes_per_forward": fwd_bytes,
                                "achieved": fwd_bytes / (1e9 * rt / a.rollout_steps), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": fwd_bytes / (1e9 * rt / a.rollout_steps) / HBM_PEAK_GBS}}

    # ---- the same rollout on the OPT-IN f16x2 eval arithmetic (FNO3d.set_arith: two fp16 planes per operand, three products, dropped term
    #      <= 2^-22 |a b| -- below the fp32 grade of the line above, which stays the headline): a labelled secondary line with its error
    rollout_h2 = None
    if rollout is not None and world == 1:
        try:
            ref_out = autoregressive_rollout(model, x, a.rollout_steps).clone()
            model.set_arith("f16x2")
            out_h2 = autoregressive_rollout(model, x, a.rollout_steps)          # warm-up at full length
            err = float(torch.linalg.vector_norm((out_h2 - ref_out).double()) / torch.linalg.vector_norm(ref_out.double()))
            err1 = float(torch.linalg.vector_norm((out_h2[:, :shape[0]] - ref_out[:, :shape[0]]).double())
                         / torch.linalg.vector_norm(ref_out[:, :shape[0]].double()))
            del ref_out, out_h2
            rts2 = []
            for _ in range(3):
                barrier()
                t0 = time.perf_counter()
                autoregressive_rollout(model, x, a.rollout_steps)
                barrier()
                rts2.append(time.perf_counter() - t0)
            rt2 = sum(rts2) / len(rts2)
            rollout_h2 = {"value": B * shape[0] * a.rollout_steps / rt2, "unit": "fields/s", "ms_per_forward": 1e3 * rt2 / a.rollout_steps,
                          "ms_per_forward_min": 1e3 * min(rts2) / a.rollout_steps, "runs": len(rts2),
                          "speedup_vs_default": rt / rt2,
                          "frac": fwd_bytes / (1e9 * rt2 / a.rollout_steps) / HBM_PEAK_GBS,
                          "rel_l2_vs_default_step1": err1, f"rel_l2_vs_default_{a.rollout_steps}_steps": err,
                          "arithmetic": "OPT-IN (FNO3d.set_arith('f16x2')): eval cell_mix launches and the head with operands as two fp16 "
                                        "planes (RNE, one fp32 ulp), three products per fp32 product, dropped term <= 2^-22 |a b|; "
                                        "NOT the headline: the default rollout above drops <= 2^-24",
                          "tolerance": "stated by this repo: Rel-L2 vs the default path < 5e-6 per forward (tests/test_gpu_f16x2.py)"}
        except Exception as e:                                  # must never cost the bench line
            rollout_h2 = {"error": repr(e)}
        finally:
            model.set_arith("f32")

    # ---- the STRONG parity guard (the loss equality above is a weak discriminator -- with N(0,1) targets an error that is
    #      uncorrelated with the target moves the loss at second order): one fused Trainer.step at the headline shape, B = 2, through the same
    #      kernels, against what the IMPORTED reference produced for the same seeded weights and batch -- the Frobenius norm and 256 sampled
    #      entries of EVERY parameter gradient (tests/golden/fno3d_headline.npz, b2/*; tests/test_gpu_headline.py holds the same check)
    grad_check = None
    if a.full and world == 1 and rank == 0 and not a.only_headline:
        try:
            import numpy as np
            sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
            import headline_common as HC
            gz = np.load(os.path.join(ROOT, "tests", "golden", "fno3d_headline.npz"))
            sd2 = HC.headline_state_dict()
            x2, y2 = HC.headline_batch(2)
            same = (np.allclose(HC.checksum(x2), gz["b2/x_checksum"], rtol=1e-12, atol=1e-9)
                    and np.allclose(HC.checksum(y2), gz["b2/y_checksum"], rtol=1e-12, atol=1e-9)
                    and np.allclose(np.array([HC.checksum(v) for k, v in sorted(sd2.items()) if v.dtype != torch.int64]), gz["b2/w_checksum"],
                                    rtol=1e-12, atol=1e-9))
            if not same:
                grad_check = {"skipped": "the seeded streams differ on this host: fixture not applicable"}
            else:
                m2 = FNO3d(*HC.MODES, HC.N_LAYERS, HC.WIDTH, HC.SHAPE, HC.SHAPE)
                m2.load_state_dict(sd2)
                m2 = m2.to(dev)
                tr2 = Trainer(m2, lr=0.0, num_update=4000)
                l2 = float(tr2.step(x2.to(dev), y2.to(dev)))
                grads = m2.grads_as_state_dict(tr2.grad)
                names = [k[len("b2/gnorm/"):] for k in gz.files if k.startswith("b2/gnorm/")]
                worst_n = worst_s = 0.0
                worst_n_name = worst_s_name = ""
                for k in names:
                    g = grads[k].cpu()
                    g = torch.view_as_real(g) if g.is_complex() else g
                    if k.startswith("convs.") and k.endswith(".bias"):       # true gradient 0 (BatchNorm cancels it): noise on both sides
                        continue
                    gn = float(gz[f"b2/gnorm/{k}"])
                    en = abs(float(g.double().norm()) - gn) / gn
                    samp = g.flatten()[HC.sample_index(g.numel(), k)].double()
                    rs = torch.from_numpy(gz[f"b2/gsamp/{k}"]).double()
                    es = float(torch.linalg.vector_norm(samp - rs) / torch.linalg.vector_norm(rs))
                    if en > worst_n:
                        worst_n, worst_n_name = en, k
                    if es > worst_s:
                        worst_s, worst_s_name = es, k
                lref = float(gz["b2/loss"])
                grad_check = {"tensors": len(names), "max_rel_err_of_gradient_norms": worst_n, "max_rel_l2_of_256_samples": worst_s,
                              "worst_norm_tensor": worst_n_name, "worst_samples_tensor": worst_s_name,
                              "loss_rel_err": abs(l2 - lref) / abs(lref), "tol_norms": 5e-5, "tol_samples": 2e-4,
                              "fatal_above": "10 x the tolerances (the test suite holds the tolerances themselves; fp32 CPU autograd of the "
                                             "reference carries ~1e-5 on the smallest gradients)",
                              "source": "tests/golden/fno3d_headline.npz b2/* (imported reference, headline shape, B = 2, same seeds)"}
                del m2, tr2, grads
                torch.cuda.empty_cache()
                grad_check["within_tolerance"] = bool(worst_n < 5e-5 and worst_s < 2e-4 and grad_check["loss_rel_err"] < 1e-5)
                if not (worst_n < 5e-4 and worst_s < 2e-3 and grad_check["loss_rel_err"] < 1e-4):
                    raise SystemExit(f"bench.py: gradient check against the reference fixture failed ({grad_check}); refusing to report a number")
        except SystemExit:
            raise
        except Exception as e:                                  # a missing fixture must not cost the bench line
            grad_check = {"error": repr(e)}

    extra = {}
    proxy = None
    if world == 1:
        model = None
        torch.cuda.empty_cache()
        if not a.no_scaling_proxy and not force_dp:
            # In its OWN process: the N-rank run the proxy stands for starts its data-parallel path in a fresh process too, and a process
            # that has run the single-GPU sections first measures the DP steps differently (round 6: +4 .. +6 ms per step, DESIGN.md
            # section 6).  This process frees its headline model first; the child reports a JSON object.
            try:
                import subprocess
                trainer = x = y = None
                torch.cuda.empty_cache()
                env = dict(os.environ, MASTER_PORT="29517")
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--proxy-worker", repr(float(ms_per_step))],
                                   capture_output=True, text=True, timeout=900, env=env)
                lines = [ln for ln in r.stdout.split("\n") if ln.startswith("PROXY_JSON ")]
                if not lines:
                    raise RuntimeError(f"proxy worker rc {r.returncode}: {r.stderr[-400:]}")
                proxy = json.loads(lines[-1][len("PROXY_JSON "):])
                proxy["process"] = "child process of bench.py (fresh HIP context), started after the timed regions"
            except Exception as e:                          # must never cost the bench line
                proxy = {"error": repr(e)}
        for name, fn, flag in (("fno_native", bench_fno_native, a.no_fno_native), ("fno_fsi", bench_fno_fsi, a.no_fno_native),
                               ("rollout_bf16", bench_rollout_bf16, a.no_bf16),
                               ("transolver", bench_transolver, a.no_transolver), ("transolver_b16", bench_transolver_b16, a.no_transolver),
                               ("transolver_c4", bench_transolver_c4, a.no_transolver),
                               ("galerkin_transformer", bench_galerkin, a.no_galerkin), ("dpot_s", bench_dpot, a.no_dpot),
                               ("unet", bench_unet, a.no_unet),
                               ("unet_c3", bench_unet_c3, a.no_unet)):
            if not flag:
                try:
                    extra[name] = fn(dev)
                except AssertionError as e:                 # a secondary block must not take the headline line down
                    extra[name] = {"error": str(e)}
    rccl_ranks = dist.get_world_size() if (world > 1 or force_dp) else 1
    if world > 1 or force_dp:
        torch.cuda.synchronize()
        _flush_c_stdio()                                    # every rank empties its C stdio buffer (RCCL banner) ...
        dist.barrier()                                      # ... before rank 0 goes on to print the JSON line
        if model is not None and getattr(model, "dp", None) is not None:
            model.dp.close()                                # RCCL communicators go before the process group does
        dist.destroy_process_group()

    if rank == 0:
        ach_gbs = dom["bytes"] / dom["total_ms"] / 1e6
        ach_tf = dom["flops"] / dom["total_ms"] / 1e9
        per_launch = dom["bytes"] / dom["calls"]
        step_bytes = (6.238 * B + 4.03) * 1e9          # algorithmic bytes of one train step
        traffic = traffic_src = None                    # HBM bytes per launch of the dominant family: measured now with --pmc
        if not a.no_pmc and B == 32 and world == 1 and not force_dp:      # (two rocprofv3 counter passes over the kernel micro-benchmark) ...
            traffic, traffic_src = live_pmc_traffic(dominant)
        if traffic is None:                             # ... else from the committed passes of the same kernels
            try:
                tj = json.load(open(os.path.join(ROOT, "profiles", "traffic_per_launch.json")))
                if B == 32:
                    traffic = tj["bytes_per_launch"].get(dominant)
                    traffic_src = tj.get("source")
            except Exception:
                pass
        line = {
            "metric": "train-step samples/sec (+ autoregressive rollout fields/sec in 'rollout'), FNO cylinder 128^2",
            "value": value, "unit": "samples/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": a.scaling, "vs_baseline": None,
            "dtype": "f32 storage / split-bf16x3 MFMA contractions (six bf16 products per fp32 product, fp32 accumulate), fp32-grade",
            "data": "synthetic",
            "config": {"workload": "FNO3d train step (fwd+MSE+bwd+Adam+cosine), cylinder-shaped [B,20,128,128,2] "
                                   "-> padded 26x134x134, modes (4,12,16), width 64, 4 layers (BASELINE.json configs[1])",
                       "batch_per_gpu": B, "global_batch": B * world, "scaling": a.scaling,
                       "parallelism": f"dp{world}" if world > 1 else "single",
                       "collective": (f"{'RCCL' if backend == 'nccl' else backend} all-reduce, {rccl_ranks} rank(s)"
                                      if backend else None)},
            "roofline": {"bound": "hbm", "kernel": dominant + " (all template variants, aggregated)",
                         "achieved": ach_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": ach_gbs / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                         "traffic_note": "PMC request-size bytes per launch of the same kernels at the same sizes, collected over the "
                                         "kernel micro-benchmark tools/kbench.py (not inside the timed step)",
                         "avg_launch_ms": dom["total_ms"] / dom["calls"], "launches_timed": dom["calls"],
                         "launches_per_step": dom["calls"] / a.steps,
                         "family_ms_per_step": dom["total_ms"] / a.steps,
                         "family_share_of_step": dom["total_ms"] / a.steps / ms_per_step,
                         "algorithmic_bytes_per_launch": per_launch,
                         "variants": dom["variants"],
                         "mfma_f32": {"achieved": ach_tf, "peak": MFMA_F32_PEAK_TF, "unit": "TFLOP/s",
                                      "frac": ach_tf / MFMA_F32_PEAK_TF},
                         "whole_step": {"algorithmic_bytes": step_bytes,
                                        "achieved": step_bytes / (ms_per_step * 1e6), "unit": "GB/s",
                                        "frac": step_bytes / (ms_per_step * 1e6) / HBM_PEAK_GBS}},
            # the second half of BASELINE.json's metric, first class (details in "rollout")
            "rollout_value": rollout["value"] if rollout else None, "rollout_unit": "fields/s",
            "rollout_ms_per_forward": rollout["ms_per_forward"] if rollout else None,
            "rollout_frac": rollout["roofline"]["frac"] if rollout else None,
            "rollout": rollout,
            "rollout_f16x2": rollout_h2,
            "loss": float(loss),
            "first_step_loss": first_loss_global,
            "loss_check": loss_check,
            "grad_check": grad_check,
        }
        if ceiling:
            # which mix each cell_mix variant streams: forward = 1 read + 1 write (+ the small z2 rows), backward with the BatchNorm
            # sums = 2 reads + 1 write; the family figure weights them by time
            best = max(ceiling.values())
            fam_floor = sum(v["algorithmic_bytes_per_launch"] * v["launches"] / a.steps /
                            ceiling["r2w1" if "stats=2" in k else "r1w1"] / 1e6 for k, v in dom["variants"].items())
            kern_floor = sum(v["bytes"] * v["calls"] / max(a.warmup, 1) for v in warm.values()) / best / 1e6
            line["roofline"].update(
                copy_ceiling={"GBps": ceiling, "frac_of_peak": {k: v / HBM_PEAK_GBS for k, v in ceiling.items()},
                              "how": "csrc/rpb_probe.hip: plain streaming kernel (nontemporal loads / stores, the policy of the product kernels since round 5), "
                                     "3.82 GB tensors, 16 B per lane, best of 256 / 512 threads; "
                                     "measured in this run after the timed region"},
                frac_of_copy_ceiling=fam_floor / (dom["total_ms"] / a.steps),
                floor_ms={"dominant_family_at_copy_ceiling": fam_floor,
                          "whole_step_kernels_at_copy_ceiling": kern_floor,
                          "whole_step_survey_byte_model_at_copy_ceiling": step_bytes / best / 1e6,
                          "note": "a step that moved every algorithmic byte exactly once at the rate a plain copy reaches on this chip; "
                                  "kernels = sum over this step's launches of their own algorithmic bytes (layer-0 algebra and the fused "
                                  "head move fewer bytes than SURVEY's model)"})
            line["roofline"]["whole_step"]["frac_of_copy_ceiling"] = step_bytes / (ms_per_step * 1e6) / best
        if mfma_peak:
            for v in extra.values():                        # the secondary models' split-bf16 pipe fraction against the measured ceiling
                sp = (v.get("roofline") or {}).get("split_bf16_mfma") if isinstance(v, dict) else None
                if sp:
                    sp["frac_of_sustained_rate"] = sp["achieved"] / (mfma_peak["random_operands"] / 6.0)
            line["mfma_bf16_sustained"] = {"TFLOPs": mfma_peak, "datasheet_peak": MFMA_BF16_PEAK_TF,
                                           "frac_of_datasheet": {k: v / MFMA_BF16_PEAK_TF for k, v in mfma_peak.items()},
                                           "split_bf16_fp32_equivalent_TFLOPs": mfma_peak["random_operands"] / 6.0,
                                           # the probe issues 32x32x16 MFMAs back to back, 32 matrix-pipe cycles each on every SIMD: the rate
                                           # IS the shader clock the power management holds under that load (the
                                           # evaluation head runs at 1.06-1.53 GHz by clock64 against the 100 MHz counter)
                                           "implied_shader_clock_GHz": {k: v * 1e12 / (2.0 * 32 * 32 * 16) / (4.0 * _num_cus(dev)) * 32 / 1e9
                                                                        for k, v in mfma_peak.items()},
                                           "how": "csrc/rpb_probe.hip: 4 independent v_mfma_f32_32x32x16_bf16 chains per wave, one wave per SIMD, "
                                                  "register operands; measured in this run.  The secondary models' split-bf16 kernels move real "
                                                  "(random-like) data: their ceiling is the random-operand rate, not the datasheet's"}
        if rollout:                                          # the second half of the metric, inside the dict the driver's record keeps whole
            line["roofline"]["rollout"] = {"value": rollout["value"], "unit": "fields/s", "ms_per_forward": rollout["ms_per_forward"],
                                           "ms_per_forward_min": rollout["ms_per_forward_min"], "runs": rollout["runs"],
                                           "achieved": rollout["roofline"]["achieved"], "frac": rollout["roofline"]["frac"]}
        # FLAT scalars: the driver's record keeps the scalar fields of `roofline` and drops nested dicts
        rf = line["roofline"]
        rf["whole_step_frac"] = rf["whole_step"]["frac"]
        rf["whole_step_GBps"] = rf["whole_step"]["achieved"]
        rf["whole_step_algorithmic_GB"] = step_bytes / 1e9
        if rollout:
            rf["rollout_fields_per_s"] = rollout["value"]
            rf["rollout_ms_per_forward"] = rollout["ms_per_forward"]
            rf["rollout_frac"] = rollout["roofline"]["frac"]
            rf["rollout_GBps"] = rollout["roofline"]["achieved"]
        if rollout_h2 and "error" not in rollout_h2:            # opt-in secondary arithmetic: flat, labelled by name
            rf["rollout_f16x2_optin_fields_per_s"] = rollout_h2["value"]
            rf["rollout_f16x2_optin_ms_per_forward"] = rollout_h2["ms_per_forward"]
            rf["rollout_f16x2_optin_frac"] = rollout_h2["frac"]
            rf["rollout_f16x2_optin_rel_l2_vs_default"] = rollout_h2["rel_l2_vs_default_step1"]
        if loss_check:
            rf["loss_check_rel_err"] = loss_check.get("rel_err")
        if grad_check and "max_rel_err_of_gradient_norms" in grad_check:
            rf["grad_check_max_rel_err_norms"] = grad_check["max_rel_err_of_gradient_norms"]
            rf["grad_check_max_rel_l2_samples"] = grad_check["max_rel_l2_of_256_samples"]
        if dp_info:
            line["dp"] = dp_info
        if proxy:
            line["strong_scaling_proxy"] = proxy
            if isinstance(proxy, dict) and "speedup_ceiling" in proxy:
                line["roofline"]["strong_scaling_proxy_speedup_ceiling"] = proxy["speedup_ceiling"]
                sc = proxy["speedup_ceiling"]
                rf["strong_scaling_ceiling_8"] = sc.get("8_ranks")
                rf["strong_scaling_ceiling_8_sharded_adam"] = sc.get("8_ranks_sharded_adam")
                rf["strong_scaling_ceiling_8_modelled_comm"] = sc.get("8_ranks_sharded_adam_modelled_comm")
            if isinstance(proxy, dict) and "weak_scaling_modelled_efficiency_8" in proxy:
                rf["weak_scaling_modelled_efficiency_8"] = proxy["weak_scaling_modelled_efficiency_8"]
                rf["weak_scaling_modelled_efficiency_8_pessimistic"] = proxy["weak_scaling_modelled_efficiency_8_pessimistic"]
                line["weak_scaling_modelled_efficiency_8"] = proxy["weak_scaling_modelled_efficiency_8"]
        line.update(extra)
        if not a.no_cpu_baseline and world == 1:
            line["cpu_baseline"] = cpu_baseline()
        if dumped:
            line["dumped_outputs"] = dumped
        if a.record:
            os.makedirs(os.path.dirname(os.path.abspath(a.record)), exist_ok=True)
            with open(a.record, "w") as f:
                json.dump(line, f)
                f.write("\n")
        sys.stdout.flush()
        _flush_c_stdio()
        print(json.dumps(compact_line(line)), flush=True)   # the ONE JSON line, last thing on stdout


if __name__ == "__main__":
    main()
