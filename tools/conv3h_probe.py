#!/usr/bin/env python
"""A/B of the opt-in f16x2 convolution arithmetic (csrc/rpb_conv3h.hip) against the default bf16x3 path at the cylinder configs.

  python tools/conv3h_probe.py                   # eval forwards + 3-step rollouts of Transolver (B = 4) and Unet3d (B = 12),
                                                 # both arithmetics alternated twice in one process, same seeded inputs; Rel-L2 between them
  python tools/conv3h_probe.py --kernels         # the convolutions alone at the Transolver (256 -> 512) and U-Net (64 / 128 / 256)
                                                 # shapes, both arithmetics (run under rocprofv3 --kernel-trace for per-launch times)
  python tools/conv3h_probe.py --summarize DIR   # per-launch table of conv3x / conv3x_f16x2 from the *_kernel_trace.csv under DIR
"""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, H, W = 20, 64, 128                                   # configs/cylinder: shape_in [20, 64, 128, 3]


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps, out


def models(ub):
    import torch
    from realpdebench_amd.model.transolver import Transolver
    from realpdebench_amd.model.unet import Unet3d
    torch.manual_seed(0)
    tr = Transolver(space_dim=3, n_layers=1, n_hidden=256, n_head=8, fun_dim=0, out_dim=3, slice_num=16, mlp_ratio=4, ref=4,
                    H=W, W=H, D=T, dropout=0.1).cuda().eval()          # configs/cylinder/trainsolver.yaml (H, W, D = 128, 64, 20)
    un = Unet3d(dim=H, out_channels=3, dim_mults=[1, 2, 4], channels=3, in_time=T, out_time=T).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    xt = torch.randn(4, T, H, W, 3, device="cuda", generator=g)
    xu = torch.randn(ub, T, H, W, 3, device="cuda", generator=g)
    return [("transolver", tr, xt), ("unet", un, xu)]


def ab(args):
    import torch
    from realpdebench_amd.rollout import autoregressive_rollout
    print(f"# conv3h_probe A/B: cylinder configs (T, H, W) = {(T, H, W)}, {args.reps} timed reps after one warm-up, "
          f"f32 / f16x2 alternated twice", flush=True)
    with torch.no_grad():
        for name, m, x in models(args.unet_batch):
            outs = {}
            for rnd in range(2):
                for arith in ("f32", "f16x2"):
                    m.set_arith(arith)
                    ms_f, y = timed(lambda: m(x), args.reps)
                    ms_r, r = timed(lambda: autoregressive_rollout(m, x, 3), max(1, args.reps // 2))
                    outs[arith] = (y, r)
                    print(f"{name:10s} B={x.shape[0]:2d} round {rnd} {arith:5s}: eval forward {ms_f:8.2f} ms   rollout(3) {ms_r:8.2f} ms",
                          flush=True)
            print(f"{name:10s} Rel-L2 f16x2 vs f32: forward {rel(outs['f16x2'][0], outs['f32'][0]):.3e}   "
                  f"rollout(3) {rel(outs['f16x2'][1], outs['f32'][1]):.3e}", flush=True)
            m.set_arith("f32")
            del m, x, outs
            torch.cuda.empty_cache()


# (label, B, mesh, Ci, Co): the Transolver block convolution (in_project_fx | in_project_x fused) and the U-Net levels (B = 12)
SHAPES = [("transolver 256->512", 4, (W, H, T), 256, 512), ("unet 64->64", 12, (T, H, W), 64, 64),
          ("unet 128->128", 12, (T, H // 2, W // 2), 128, 128), ("unet 256->256", 12, (T, H // 4, W // 4), 256, 256)]


def kernels(args):
    import torch
    from realpdebench_amd import ops
    for label, B, mesh, Ci, Co in SHAPES:
        M = B * mesh[0] * mesh[1] * mesh[2]
        torch.manual_seed(Ci + Co)
        x = torch.randn(M, Ci, device="cuda")
        w = torch.randn(Co, 27 * Ci, device="cuda") / (27 * Ci) ** 0.5
        b = torch.randn(Co, device="cuda")
        wh = ops.conv3_f16x2_weights(w, Co, Ci)
        ys = {}
        for arith in ("f32", "f16x2"):
            y = torch.empty(M, Co, device="cuda")
            for _ in range(args.reps):
                ops.conv3(x, w, y, M, Co, Ci, mesh, bias=b, arith=arith, wh=wh if arith == "f16x2" else None)
            ys[arith] = y
        torch.cuda.synchronize()
        print(f"{label:22s} M={M:8d}  Rel-L2 f16x2 vs f32 {rel(ys['f16x2'], ys['f32']):.3e}", flush=True)
        del x, w, ys, wh
        torch.cuda.empty_cache()


def summarize(path):
    """Mean per-launch time of the two convolution kernels, keyed by (kernel, grid): every shape of SHAPES has its own grid."""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    rows = {}
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                n = r.get("Kernel_Name", "")
                if "conv3x_kernel" not in n and "conv3x_f16x2_kernel" not in n:
                    continue
                grid = tuple(int(r.get(k, 0) or 0) for k in ("Grid_Size_X", "Grid_Size_Y")) if "Grid_Size_X" in r else (int(r.get("Grid_Size", 0)),)
                kind = "conv3x_f16x2" if "f16x2" in n else "conv3x"
                inst = n[n.index("<"):n.index(">") + 1] if "<" in n else ""
                rows.setdefault((grid, kind, inst), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    print(f"# per-launch times of conv3x (default, bf16x3) and conv3x_f16x2 from {len(files)} rocprofv3 kernel trace(s)")
    print(f"{'kernel':14s} {'instance':10s} {'grid':>16s} {'launches':>8s} {'mean_us':>10s} {'min_us':>10s}")
    for (grid, kind, inst), ds in sorted(rows.items()):
        print(f"{kind:14s} {inst:10s} {str(grid):>16s} {len(ds):8d} {sum(ds) / len(ds) / 1e3:10.1f} {min(ds) / 1e3:10.1f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--unet-batch", type=int, default=12)
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.kernels:
        kernels(a)
    else:
        ab(a)
