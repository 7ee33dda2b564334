"""SyncBN for the two BatchNorm models of the ArenaTrainer, CNO3d and DeepONet (``enable_training(sync_bn=True)``), on ONE MI355X: two
ranks share cuda:0 and reduce through gloo, as in tests/test_gpu_dp.py (RCCL refuses two ranks on one device).

The contract is "N ranks with B / N samples each take the step one rank takes on all B samples", and the one-rank step is pinned by the
fixtures of the reference's fp64 run (tests/golden/cno_train_small.npz, deeponet_train_small.npz): every rank gets ONE sample of a B = 2
case, and what the two ranks hold after the step -- the rank-averaged gradients, the running statistics, the mean of the two losses --
is compared with the fixture of the whole batch under the rule of tests/cno_train_helpers.py / tests/deeponet_train_helpers.py:
Rel-L2 < max(1e-5, 4 x the reference's own fp32-vs-fp64 deviation).  Per-sample statistics differ from the batch's by about
1 / sqrt(M_local) -- 7 % at M = 192 --, so a path that skips one reduction misses that rule by orders of magnitude.

The one-rank proxy (RPB_DP_SYNCBN_ALWAYS=1 on an initialised one-rank group: every reduction and both SyncBN kernels run, the sums are
over one rank) must leave the bits of the plain step.

Measured on an MI355X.  CNO3d case g: worst sampled gradient / gradient norm at 0.49 / 0.07 of their bounds, worst running statistic at
0.014, mean of the ranks' losses 1.6e-8 (step 0) and 2.2e-6 (step 1) against 1e-5.  DeepONet case a: 0.31 / 0.14, 0.007, losses 7.5e-7
and 5.9e-7; case d (dropout masks): 0.33 / 0.07, 0.006, loss 1.5e-7.  The proxy: bit-equal, 62 and 8 reductions."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(worker, world, *args):
    port = _free_port()
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(worker, args=(world, port, *args, out), nprocs=world, join=True)
        return {k: v for k, v in out.items()}


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)


def _helpers(family):
    if family == "cno":
        import cno_train_common as TC
        import cno_train_helpers as H
    else:
        import deeponet_train_common as TC
        import deeponet_train_helpers as H
    return TC, H


def _snapshot(m, tr):
    """what one rank holds after a step, on the host: the rank-averaged gradients by name, the buffers by name"""
    torch.cuda.synchronize()
    grads = tr.mean_grads()
    return ({n: grads[p].detach().cpu().clone() for n, p in m.named_parameters() if p in grads},
            {n: b.detach().cpu().clone() for n, b in m.named_buffers()})


def _two_rank_worker(rank, world, port, family, out):
    """One sample per rank of the family's B = 2 Adam case, ADAM_STEPS steps; DeepONet: then one step of case d on the explicit masks."""
    _init(rank, world, port)
    try:
        from realpdebench_amd.trainer import ArenaTrainer, make_trainer
        TC, H = _helpers(family)
        case = TC.ADAM_CASE
        res = {}
        plain = H.new_model(case).to(DEV).enable_training()
        try:                                                             # without the flag: still refused, with the class's words
            make_trainer(plain, lr=TC.ADAM_LR, num_update=TC.ADAM_T_MAX)
            res["refusal"] = None
        except NotImplementedError as e:
            res["refusal"] = (str(e), plain.DP_MSG)
        m = H.new_model(case).to(DEV).enable_training(sync_bn=True).train()
        tr = make_trainer(m, lr=TC.ADAM_LR, num_update=TC.ADAM_T_MAX)
        assert isinstance(tr, ArenaTrainer) and tr.world == world and m.bn_sync is not None and m.bn_sync.world_size == world
        res["losses"] = []
        for k in range(TC.ADAM_STEPS):
            x, y = TC.case_inputs(case, k)
            assert x.shape[0] == world, "one sample per rank"
            res["losses"].append(float(tr.step(x[rank:rank + 1].to(DEV), y[rank:rank + 1].to(DEV))))
            if k == 0:
                res["grads0"], res["buffers0"] = _snapshot(m, tr)
        torch.cuda.synchronize()
        res["flat"], res["buffers"] = tr.flat.cpu(), _snapshot(m, tr)[1]
        if family == "deeponet":                                         # dropout 0.1 through the explicit masks: the rank's own rows
            case = "d"
            B, N = TC.CASES[case][3], TC.CASES[case][1][0] * TC.CASES[case][0][1] * TC.CASES[case][0][2]
            assert B == world
            m = H.new_model(case).to(DEV).enable_training(seed=1234, sync_bn=True).train()
            m0, m1, m2 = TC.dropout_masks(case)
            m._mask_override = [m0[rank:rank + 1].to(DEV), m1[rank * N:(rank + 1) * N].to(DEV), m2[rank * N:(rank + 1) * N].to(DEV)]
            tr = make_trainer(m, lr=TC.ADAM_LR, num_update=TC.ADAM_T_MAX)
            x, y = TC.case_inputs(case)
            res["d_loss"] = float(tr.step(x[rank:rank + 1].to(DEV), y[rank:rank + 1].to(DEV)))
            res["d_grads"], res["d_buffers"] = _snapshot(m, tr)
        out[rank] = res
    finally:
        dist.destroy_process_group()


def _check_step(family, case, grads, buffers, loss, gold_loss, gold_loss_selferr, tracked):
    """the rank-averaged gradients, the running statistics and the mean loss of one step against the fixture of the whole batch"""
    TC, H = _helpers(family)
    report = []
    if family == "cno":
        *worst, misses = H.compare_gradients(case, grads, H.tol, report)
    else:
        *worst, misses = H.compare_gradients(case, grads, report)
    print("\n".join(report))
    print(f"{family} case {case}: worst gradient samples / norm at {worst[0]:.2f} / {worst[1]:.2f} of their bounds")
    worst_stat, stat_misses = 0.0, []
    for j, (k, sl) in enumerate(H.stat_slices(case).items()):
        e, bound = H.rel(buffers[k], H.GOLD[f"{case}_stats"][sl]), H.tol(H.GOLD[f"{case}_stats_selferr"][j])
        worst_stat = max(worst_stat, e / bound)
        if not e < bound:
            stat_misses.append((k, e, bound))
    el, bl = abs(loss - float(gold_loss)) / float(gold_loss), H.tol(gold_loss_selferr)
    print(f"{family} case {case}: worst running statistic at {worst_stat:.3f} of its bound; mean of the ranks' losses rel {el:.2e} (tol {bl:.1e})")
    assert not misses, misses
    assert not stat_misses, stat_misses
    assert el < bl
    counters = [int(v) for k, v in buffers.items() if k.endswith("num_batches_tracked") and not k.startswith("decoder_inv.3.")]
    assert len(counters) == tracked and all(v == TC.TRACKED_BEFORE + 1 for v in counters), "num_batches_tracked == 8"


def _check_two_ranks(family, res):
    TC, H = _helpers(family)
    case = TC.ADAM_CASE
    for r in (0, 1):
        said, msg = res[r]["refusal"]
        assert said == msg and "SyncBN" in said and "one rank" in said and "sync_bn" in said, "without the flag make_trainer refuses two ranks"
    # the ranks hold the same rank-averaged gradients; after every step the same parameters and buffers, bit for bit
    for n, g in res[0]["grads0"].items():
        assert torch.equal(g, res[1]["grads0"][n]), n
    assert torch.equal(res[0]["flat"], res[1]["flat"])
    for n, b in res[0]["buffers"].items():
        assert torch.equal(b, res[1]["buffers"][n]), n
    losses = [0.5 * (res[0]["losses"][k] + res[1]["losses"][k]) for k in range(TC.ADAM_STEPS)]
    _check_step(family, case, res[0]["grads0"], res[0]["buffers0"], losses[0], H.GOLD[f"{case}_adam_loss"][0], H.GOLD[f"{case}_adam_loss_selferr"][0],
                31 if family == "cno" else 4)
    for k in range(1, TC.ADAM_STEPS):
        e, bound = abs(losses[k] - float(H.GOLD[f"{case}_adam_loss"][k])) / float(H.GOLD[f"{case}_adam_loss"][k]), H.tol(H.GOLD[f"{case}_adam_loss_selferr"][k])
        print(f"{family} case {case} step {k}: mean of the ranks' losses rel {e:.2e} (tol {bound:.1e})")
        assert e < bound
    assert abs(res[0]["losses"][0] - res[1]["losses"][0]) > 1e-4 * losses[0], "the ranks saw different samples"


def test_cno_two_ranks_take_the_step_of_the_whole_batch():
    """CNO3d case g (B = 2, the fixture's Adam case), one sample per rank, ADAM_STEPS steps through make_trainer."""
    _check_two_ranks("cno", _spawn(_two_rank_worker, 2, "cno"))


def test_deeponet_two_ranks_take_the_step_of_the_whole_batch():
    """DeepONet case a (B = 2, dropout 0, the Adam case) likewise; then case d (dropout 0.1): one step with each rank on its own rows
    of the explicit masks, against the fixture of the whole batch."""
    res = _spawn(_two_rank_worker, 2, "deeponet")
    _check_two_ranks("deeponet", res)
    TC, H = _helpers("deeponet")
    for n, g in res[0]["d_grads"].items():
        assert torch.equal(g, res[1]["d_grads"][n]), n
    _check_step("deeponet", "d", res[0]["d_grads"], res[0]["d_buffers"], 0.5 * (res[0]["d_loss"] + res[1]["d_loss"]), H.GOLD["d_loss"],
                H.GOLD["d_loss_selferr"], 4)


# ----------------------------------------------------------------------------------------------------------- the one-rank proxy
def _proxy_worker(rank, world, port, out):
    os.environ["RPB_DP_SYNCBN_ALWAYS"] = "1"
    _init(rank, world, port)
    try:
        from realpdebench_amd.trainer import make_trainer
        res = {}
        for family, case, layers in (("cno", "d", 31), ("deeponet", "c", 4)):
            TC, H = _helpers(family)
            x, y = (t.to(DEV) for t in TC.case_inputs(case))
            held = {}
            for kind in ("plain", "sync"):
                m = H.new_model(case).to(DEV).enable_training(**({"sync_bn": True} if kind == "sync" else {})).train()
                tr = make_trainer(m, lr=1e-3, num_update=10)
                calls = []
                if kind == "sync":                                   # count the reductions: two per BatchNorm layer and step
                    reduce = m.bn_sync.all_reduce_sum
                    m.bn_sync.all_reduce_sum = lambda t, reduce=reduce, calls=calls: (calls.append(t.numel()), reduce(t))[1]
                else:
                    assert m.bn_sync is None, "an instance enabled without the flag gets no StatsSync"
                loss = tr.step(x, y)
                torch.cuda.synchronize()
                held[kind] = dict(flat=tr.flat.cpu(), grad=tr.grad.cpu(), loss=loss.cpu(), buffers={n: b.cpu() for n, b in m.named_buffers()},
                                  calls=calls)
            p, s = held["plain"], held["sync"]
            res[family] = dict(calls=s["calls"], layers=layers, flat=torch.equal(p["flat"], s["flat"]), grad=torch.equal(p["grad"], s["grad"]),
                               loss=torch.equal(p["loss"], s["loss"]), moved=bool(s["grad"].any()),
                               buffers=[n for n, b in p["buffers"].items() if not torch.equal(b, s["buffers"][n])])
        out[rank] = res
    finally:
        dist.destroy_process_group()


def test_one_rank_proxy_leaves_the_bits_of_the_plain_step():
    """An initialised one-rank group with RPB_DP_SYNCBN_ALWAYS=1: one step of a syncing instance -- every reduction, rowbn_finish_sums and
    rowbn_act_bwd_apply_sync in every BatchNorm layer -- leaves the parameter arena, the gradient arena and the buffers of a plain enabled
    instance stepped in the same process.  CNO3d case d (B = 3, M = 720); DeepONet case c (p = 256; C = 256 runs as two halves)."""
    res = _spawn(_proxy_worker, 1)[0]
    for family, r in res.items():
        assert len(r["calls"]) == 2 * r["layers"], f"{family}: {len(r['calls'])} reductions, two per BatchNorm layer expected"
        assert r["moved"] and r["flat"] and r["grad"] and r["loss"] and not r["buffers"], (family, {k: v for k, v in r.items() if k != "calls"})
    assert sorted(set(res["deeponet"]["calls"])) == [64, 128, 256, 512], "DeepONet: the two 128-wide halves of C = 256 travel in one reduction"
