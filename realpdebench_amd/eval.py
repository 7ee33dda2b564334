"""``python -m realpdebench_amd.eval --config ... --checkpoint_path model_XXXX.pth`` -- the reference's evaluation
entrypoint (realpdebench/eval.py): load a checkpoint, roll the model out autoregressively (eval.py:311-321) and report
the normalised MSE plus RMSE / MAE / Rel-L2 in physical units and the full ``eval_metrics`` tuple of
utils/metrics.py:24-131 (R^2, kinetic energy, radially binned Fourier errors, frequency error), computed on the device by
``realpdebench_amd.metrics`` (truncated-DFT GEMMs instead of fftn + a Python triple loop)."""
import argparse
import logging
import os
import time

import torch
from torch.utils.data import DataLoader

from .data import make_datasets
from .data_normalizer import GaussianNormalizer, IdentityNormalizer
from .metrics import eval_metrics
from .model import load_model
from .rollout import autoregressive_rollout
from .utils import add_hf_compat_flags, add_args_from_config, check_hf_compat_flags, resolve_config, set_seed, setup_logging

parser = argparse.ArgumentParser(description="Evaluation Configurations")
parser.add_argument("--config", type=str, default="configs/cylinder/fno.yaml")
parser.add_argument("--gpu", type=int, default=0)
parser.add_argument("--train_data_type", type=str, default="numerical", help="numerical | real")
parser.add_argument("--checkpoint_path", type=str, default=None)
parser.add_argument("--dataset_factory", type=str, default=None)
add_hf_compat_flags(parser)


def main(argv=None):
    args = parser.parse_args(argv)
    check_hf_compat_flags(args)
    args.config = resolve_config(args.config)
    cli_ckpt = args.checkpoint_path
    args = add_args_from_config(args)
    if cli_ckpt:
        args.checkpoint_path = cli_ckpt
    if not torch.cuda.is_available():
        raise SystemExit("realpdebench_amd.eval needs an MI355X: there is no CPU fallback path")
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    set_seed(args.seed)
    # a checkpoint_path without a directory part (DMD's literal 'no model needed') puts the results under results_path
    exp_path = (os.path.dirname(args.checkpoint_path) if args.checkpoint_path else "") or args.results_path
    os.makedirs(exp_path, exist_ok=True)
    setup_logging(exp_path, is_train=False)

    train_dataset, test_dataset, stats = make_datasets(args, for_eval=True)
    loader = DataLoader(test_dataset, batch_size=args.test_batch_size, shuffle=False, num_workers=args.num_workers)
    normalizer = GaussianNormalizer(*stats, device=device) if args.normalizer == "gaussian" else IdentityNormalizer(device)
    model = load_model(train_dataset, device=device, **vars(args))
    if args.checkpoint_path:
        meta = model.load_checkpoint(args.checkpoint_path, device)                     # eval.py:284
        logging.info(f"Checkpoint {args.checkpoint_path} loaded (iteration {meta['iteration']}).")
    # optional YAML keys (not in the reference; both default to the parity path): `eval_storage: bf16` stores the activations between
    # kernels as bf16 (FNO3d at width 64; BASELINE.json configs[4]), `eval_arith:` is `Model.set_arith` (every model has it; the class
    # docstring of each says what it moves)
    for key, setter in (("eval_storage", "set_storage"), ("eval_arith", "set_arith")):
        val = getattr(args, key, None)
        if val:
            if not hasattr(model, setter):
                raise SystemExit(f"{key}: {type(model).__name__} has no {setter} (FNO3d only)")
            getattr(model, setter)(str(val))
            logging.info(f"{key} = {val}")
    results, _, _ = evaluate(model, loader, normalizer, int(args.N_autoregressive), args.test_batch_size)
    logging.info(f"Results saved at {exp_path}")
    return results


METRIC_NAMES = ("rmse", "mae", "rel l2 error", "r2", "ke error", "f error", "low f error", "mid f error", "high f error",
                "rel low f error", "rel mid f error", "rel high f error", "freq error")


def evaluate(model, loader, normalizer, n_ar, test_batch_size):
    """The test loop of realpdebench/eval.py:286-365 on the device: returns ``(results, pred, target)`` with the
    de-normalised rollout and targets of the whole split (``None`` when the targets cover a single step only)."""
    device = next((p.device for p in model.parameters()), None) or model.device       # a parameter-free model (DMD) says where it is
    leading = getattr(model, "PREDICTS_LEADING_CHANNELS", False)
    normalized_test_loss, n_batches, nb = 0.0, 0, 0
    pred_list, target_list = [], []
    unmeasured_c = None
    T_tgt = None
    start = time.time()
    logging.info(f"Start testing on {device}")
    for inp, tgt in loader:
        b = inp.size(0)
        T_tgt = tgt.shape[1]
        if unmeasured_c is None:                                    # eval.py:297-302: all-zero target channels of the FIRST batch
            unmeasured_c = sum(int(torch.all(tgt[..., c_] == 0)) for c_ in range(tgt.shape[-1]))
        c = tgt.shape[-1] - unmeasured_c
        c_out = tgt.shape[-1]
        para = inp[..., c_out:].contiguous() if inp.shape[-1] != c_out else None          # eval.py:304-308
        x, t = normalizer.preprocess(inp, tgt)
        pred = autoregressive_rollout(model, x, n_ar, normalizer=normalizer, para_input=para)
        if leading:                      # DMD predicts f <= C_out channels: metrics and loss run over the first c of them, as in the reference
            f = pred.shape[-1] - (para.shape[-1] if para is not None else 0)
            if c > f:                    # the reference dies here with a broadcast error (eval.py:323)
                raise ValueError(f"{type(model).__name__} predicts {f} channels but the targets have {c} measured (non-zero) channels: "
                                 "the metrics cannot cover a channel the model does not predict")
            pred = pred[..., :f].contiguous()
        else:
            pred = pred[..., :c_out].contiguous()
        if pred.shape[:-1] == t.shape[:-1]:        # real test splits carry n_ar * T_out target frames; synthetic sets only T_out
            normalized_test_loss += float(((pred[..., :c] - t[..., :c]) ** 2).reshape(b, -1).mean())       # eval.py:323
            _, p = normalizer.postprocess(x, pred)
            _, tt = normalizer.postprocess(x, t)
            pred_list.append(p)                                     # stay in HBM: the metrics run on the device (row f3)
            target_list.append(tt)
        n_batches += 1
        nb += b
    torch.cuda.synchronize()
    dt = time.time() - start
    T_out = (T_tgt // n_ar) if pred_list else T_tgt
    logging.info(f"rollout: {nb} trajectories x {n_ar} steps in {dt:.2f} s = {nb * T_out * n_ar / dt:.1f} fields/s")
    if not pred_list:
        logging.info("targets cover one step only: rollout timed, no metrics (a test split with N_autoregressive frames has them)")
        return {}, None, None
    normalized_test_loss /= n_batches
    pred, target = torch.cat(pred_list, dim=0), torch.cat(target_list, dim=0)
    eval_batch_size = test_batch_size if n_ar > 4 else pred.shape[0]                       # eval.py:346-349
    vals = eval_metrics(pred, target, c, eval_batch_size)                                   # eval.py:350-352, on the device
    logging.info("Test results: \n" + f"normalized mse loss: {normalized_test_loss:.5f}, "
                 + ", ".join(f"{n}: {float(v):.5f}" for n, v in zip(METRIC_NAMES, vals)))
    logging.info(f"Testing complete, time cost is {(time.time() - start) / 60:.2f} min")
    results = dict(zip(("normalized_mse",) + METRIC_NAMES, [normalized_test_loss] + [float(v) for v in vals]))
    results["evaluated_channels"] = c
    return results, pred, target


if __name__ == "__main__":
    main()
