"""The training driver on the GPU (needs an MI355X; -m gpu): the two new kernels against the numpy
restatement of tests/_train_data_ref.py, FlatAdam's state against torch.optim.Adam, the readers' device
samples, and python -m transmvsnet_amd.finetune end to end on small synthetic scans (train, resume, test,
two ranks)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import _train_data_ref as ref
from tests._util import golden_state_dict
from transmvsnet_amd import data, finetune, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
STAGES = ("stage1", "stage2", "stage3")


def _np(t):
    return t.detach().cpu().numpy()


def _tables(h, w, mode, crop=(512, 640)):
    rows, cols, _ = data.gt_pyramid_tables(h, w, mode, crop)
    return torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV)


# ------------------------------------------------------------------ tmvs_gt_pyramid
@pytest.mark.parametrize("h,w", [(37, 50), (128, 160), (576, 768)])
def test_gt_pyramid_bld(h, w):
    """Depth maps bitwise, masks equal, at tails (37 x 50 -> 18 x 25 and 9 x 12) and at C5's size; pixels
    exactly on each float32-rounded bound and one ulp either side of it."""
    dmin = 425.0
    dint = (935.0 - 425.0) / 192
    dend = dint * (192 - 1) + dmin  # Python floats, as the dataset class computes them
    g = np.random.default_rng(h * 1000 + w)
    depth = (380.0 + 600.0 * g.random((h, w))).astype(np.float32)  # straddles both bounds
    lo, hi = np.float32(dmin), np.float32(dend)
    plant = [lo, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(2000)), hi,
             np.nextafter(hi, np.float32(0)), np.nextafter(hi, np.float32(2000)), np.float32(0), np.float32(np.nan)]
    flat = depth.reshape(-1)
    flat[0:4 * len(plant):4] = np.array(plant, np.float32)  # row 0, columns 0, 4, ..., 28
    flat[-1] = hi
    rows, cols = _tables(h, w, "bld")
    got_d, got_m = ops.gt_pyramid(torch.from_numpy(depth).to(DEV), rows, cols, "bld", dmin, dend)
    want_d, want_m = ref.gt_pyramid_bld(depth, dmin, dend)
    for s in STAGES:
        assert _np(got_d[s]).tobytes() == want_d[s].tobytes(), s  # bitwise, NaN included
        np.testing.assert_array_equal(_np(got_m[s]), want_m[s], err_msg=s)
    assert want_m["stage3"].reshape(-1)[0] == 1 and want_m["stage3"].reshape(-1)[4] == 0  # on / below depth_min
    assert want_m["stage3"].reshape(-1)[12] == 1 and want_m["stage3"].reshape(-1)[20] == 0  # on / above depth_end
    assert 0 < want_m["stage1"].mean() < 1
    if h % 4 == 0 and w % 4 == 0:  # every real size: the nearest rule is plain striding
        for s, k in (("stage2", 2), ("stage1", 4)):
            np.testing.assert_array_equal(_np(got_d[s]).view(np.uint32), depth[::k, ::k].view(np.uint32))
            np.testing.assert_array_equal(_np(got_m[s]), want_m["stage3"][::k, ::k])


@pytest.mark.parametrize("h,w,start", [(70, 90, (1, 2)), (71, 93, (1, 3))])
def test_gt_pyramid_dtu(h, w, start):
    """prepare_img (halve, centre crop to 32 x 40) and the three scales as one gather; the mask from PNG
    values 9, 10, 11 (> 10)."""
    crop = (32, 40)
    g = np.random.default_rng(h)
    depth = (425.0 + 500.0 * g.random((h, w))).astype(np.float32)
    png = g.choice(np.array([9, 10, 11], np.uint8), size=(h, w))
    assert ((h // 2 - crop[0]) // 2, (w // 2 - crop[1]) // 2) == start
    rows, cols = _tables(h, w, "dtu", crop)
    got_d, got_m = ops.gt_pyramid(torch.from_numpy(depth).to(DEV), rows, cols, "dtu",
                                  mask_png=torch.from_numpy(png).to(DEV), target_hw=crop)
    want_d, want_m = ref.gt_pyramid_dtu(depth, png, crop)
    for s, k in zip(STAGES, (4, 2, 1)):
        assert tuple(got_d[s].shape) == (crop[0] // k, crop[1] // k)
        np.testing.assert_array_equal(_np(got_d[s]).view(np.uint32), want_d[s].view(np.uint32), err_msg=s)
        np.testing.assert_array_equal(_np(got_m[s]), want_m[s], err_msg=s)
    if h % 2 == 0 and w % 2 == 0:  # an even size halves by plain striding
        np.testing.assert_array_equal(want_m["stage3"],
                                      png[::2, ::2][start[0]:start[0] + 32, start[1]:start[1] + 40] == 11)
    with pytest.raises(ValueError):
        ops.gt_pyramid(torch.from_numpy(depth).to(DEV), rows, cols, "dtu", mask_png=torch.from_numpy(png).to(DEV),
                       target_hw=(h // 2 + 1, 40))
    # the C entry itself refuses the crop too (before any launch)
    from transmvsnet_amd import _lib
    d = torch.from_numpy(depth).to(DEV)
    p = d.data_ptr()
    assert _lib.load().tmvs_gt_pyramid(_lib.GT_DTU, p, p, h, w, 32, w // 2 + 1, 0.0, 0.0, p, p, p, p, p, p, p, p,
                                       None) == -2


# ------------------------------------------------------------------ tmvs_depth_eval_metrics
def _metric_case(h, w, seed, max_err, mask_zero=False):
    """gt on a 1/4 grid, errors on a 1/64 grid: est = gt + err and est - gt are exact in float32, so the
    planted errors 2, 4, 8, 14, 20 sit exactly on the thresholds."""
    g = np.random.default_rng(seed)
    gt = (425.0 + 0.25 * g.integers(0, 2000, (h, w))).astype(np.float32)
    err = (g.integers(0, int(max_err * 64), (h, w)) / 64.0).astype(np.float32)
    flat = err.reshape(-1)
    exact = [e for e in (2.0, 4.0, 8.0, 14.0, 20.0) if e <= max_err]
    for i, e in enumerate(exact * 3):
        if i < flat.size:
            flat[(i * 7) % flat.size] = e
    sign = np.where(g.random((h, w)) < 0.5, -1.0, 1.0).astype(np.float32)
    est = (gt + sign * err).astype(np.float32)
    assert (np.abs(est - gt) == err).all()
    mask = np.zeros((h, w), np.float32) if mask_zero else (g.random((h, w)) < 0.8).astype(np.float32)
    if not mask_zero:
        mask.reshape(-1)[[(i * 7) % flat.size for i in range(len(exact) * 3)]] = 1.0
    return est, gt, mask


@pytest.mark.parametrize("h,w,max_err,mask_zero", [(1, 1, 2.0, False), (37, 50, 30.0, False), (512, 640, 30.0, False),
                                                  (37, 50, 12.0, False), (37, 50, 30.0, True)])
def test_depth_eval_metrics(h, w, max_err, mask_zero):
    est, gt, mask = _metric_case(h, w, h + w, max_err, mask_zero)
    if (h, w) == (1, 1):
        est, mask = gt + np.float32(2.0), np.ones((1, 1), np.float32)  # one pixel, error exactly 2
    want = ref.depth_eval_metrics(est, gt, mask)
    args = [torch.from_numpy(a).to(DEV) for a in (est, gt, mask)]
    got = _np(ops.depth_eval_metrics(*args))
    again = _np(ops.depth_eval_metrics(*args))
    assert got.tobytes() == again.tobytes()  # fixed reduction order: bitwise repeatable
    print("depth_eval_metrics", (h, w), "got", got, "want", want)
    if mask_zero:
        assert np.isnan(got[:6]).all() and np.isnan(want[:6]).all()
        assert (got[6:] == 0).all()
        return
    # the fractions: exact counts, so the float32-rounded float64 ratio bitwise
    np.testing.assert_array_equal(got[1:6], want[1:6].astype(np.float32))
    # the means: float32 per-thread partials and the block tree, a dozen roundings of 6e-8
    for i in (0, 6, 7, 8, 9, 10, 11):
        if want[i] == 0.0:
            assert got[i] == 0.0, i
        else:
            assert abs(got[i] - want[i]) <= 1e-6 * abs(want[i]), (i, got[i], want[i])
    if (h, w) == (1, 1):  # an error of exactly 2 is not > 2 and lies in [0, 2] and in [2, 4]
        assert got[1] == 0 and got[6] == 2 and got[7] == 2 and got[8] == 0 and got[0] == 2
    elif max_err == 12.0:  # nothing above 12: the bins [14, 20] and [20, 1e5] are empty
        assert got[10] == 0 and got[11] == 0 and got[4] == 0 and got[5] == 0 and got[9] > 0
    else:
        assert (got[6:] > 0).all() and (got[1:6] > 0).all()


# ------------------------------------------------------------------ FlatAdam state
def test_flat_adam_state_continues_in_torch_adam():
    """3 FlatAdam steps on the GPU, state_dict into a CPU torch.optim.Adam, one more step on both sides:
    parameters and moments agree within test_flat_adam_matches_torch_adam's 2e-6."""
    from transmvsnet_amd.train import FlatAdam
    g = torch.Generator().manual_seed(11)
    shapes = [(8, 1, 3, 3, 3), (16,), (64, 32), (27, 8, 3, 3)]
    pg = [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in shapes]
    opt = FlatAdam(pg, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    for _ in range(3):
        opt.zero_grad()
        for p in pg:
            p.grad = (torch.randn(p.shape, generator=g) * 0.1).to(DEV)
        opt.step()
    pc = [torch.nn.Parameter(p.detach().cpu().clone()) for p in pg]
    adam = torch.optim.Adam(pc, lr=7.0, foreach=False)
    adam.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert float(adam.state[pc[0]]["step"]) == 3.0 and adam.param_groups[0]["lr"] == 1e-3
    grads = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    opt.zero_grad()
    for p, q, gr in zip(pg, pc, grads):
        p.grad, q.grad = gr.to(DEV), gr.clone()
    opt.step()
    adam.step()
    torch.cuda.synchronize()
    worst, off = 0.0, 0

    def rel(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))

    for p, q in zip(pg, pc):
        n = q.numel()
        for got, exp in ((p, q), (opt.exp_avg[off:off + n].view_as(q), adam.state[q]["exp_avg"]),
                         (opt.exp_avg_sq[off:off + n].view_as(q), adam.state[q]["exp_avg_sq"])):
            worst = max(worst, rel(got, exp))
        off += n
    print("FlatAdam state continued in torch.optim.Adam, worst relative difference:", worst)
    assert opt.step_count == 4 and float(adam.state[pc[0]]["step"]) == 4.0
    assert worst < 2e-6, worst


# ------------------------------------------------------------------ readers on the device
@pytest.fixture(scope="module")
def bld_scan(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("bld"))
    return root, synthetic.write_blended_scan(root, n_views=3, height=128, width=160)


@pytest.fixture(scope="module")
def dtu_scan(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dtu"))
    return root, synthetic.write_dtu_train_scan(root, n_views=3, height=128, width=160)


def _same_sample(got, want):
    assert got["imgs"].is_cuda and got["imgs"].dtype == torch.float32
    np.testing.assert_array_equal(_np(got["imgs"]), want["imgs"])  # float32(u8) / 255, bitwise
    for s in STAGES:
        assert got["depth"][s].is_cuda and got["mask"][s].is_cuda
        np.testing.assert_array_equal(_np(got["depth"][s]).view(np.uint32), want["depth"][s].view(np.uint32))
        np.testing.assert_array_equal(_np(got["mask"][s]), want["mask"][s])
        np.testing.assert_array_equal(got["proj_matrix"][s], want["proj_matrix"][s])
    np.testing.assert_array_equal(got["depth_values"], want["depth_values"])
    assert got["depth_interval"] == want["depth_interval"]


def test_bld_samples_on_device_match_restatement(bld_scan):
    root, listfile = bld_scan
    ds = finetune.BldTrainSet(root, listfile, "train", 3, 192, device=DEV)
    want = ref.BldRef(root, listfile, 3, 192)
    assert len(ds) == 3
    for idx in range(3):
        _same_sample(ds.sample(idx), want[idx])
    assert 0 < want[0]["mask"]["stage3"].mean() <= 1
    assert [_np(s["depth"]["stage1"]).tobytes() for s in finetune.Prefetcher(ds, [2, 0, 1])] == \
        [want[i]["depth"]["stage1"].tobytes() for i in (2, 0, 1)]


def test_dtu_samples_on_device_match_restatement(dtu_scan):
    root, listfile = dtu_scan
    ds = finetune.DtuTrainSet(root, listfile, "train", 3, 192, 1.06, device=DEV, target_hw=(128, 160))
    want = ref.DtuRef(root, listfile, 3, 192, 1.06, (128, 160))
    assert len(ds) == 21
    for idx in (0, 8, 20):
        _same_sample(ds.sample(idx), want[idx])
    m = want[0]["mask"]["stage3"]
    assert 0 < m.mean() < 1  # the PNG's 0 / 10 border is outside the mask


# ------------------------------------------------------------------ the driver end to end
@pytest.fixture(scope="module")
def golden_ckpt(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ckpt") / "golden.ckpt")
    torch.save({"model": golden_state_dict()}, path)
    return path


def _train_args(root, listfile, ckpt, logdir, epochs, *more):
    return ["--mode", "train", "--dataset", "bld_train", "--trainpath", root, "--trainlist", listfile, "--ndepths",
            "8,8,8", "--nviews", "3", "--epochs", str(epochs), "--summary_freq", "1", "--logdir", logdir,
            *(("--loadckpt", ckpt) if ckpt else ()), *more]


def _records(logdir, mode="train"):
    with open(os.path.join(logdir, "train.jsonl")) as f:
        return [r for r in map(json.loads, f) if r["mode"] == mode]


@pytest.fixture(scope="module")
def three_epochs(bld_scan, golden_ckpt, tmp_path_factory):
    root, listfile = bld_scan
    logdir = str(tmp_path_factory.mktemp("run3"))
    res = finetune.main(_train_args(root, listfile, golden_ckpt, logdir, 3))
    return logdir, res


def test_driver_three_epochs(three_epochs):
    from transmvsnet_amd import TransMVSNet
    logdir, _ = three_epochs
    assert sorted(f for f in os.listdir(logdir) if f.endswith(".ckpt")) == [f"model_00000{e}.ckpt" for e in range(3)]
    for e in range(3):
        state = torch.load(os.path.join(logdir, f"model_00000{e}.ckpt"), map_location="cpu")
        assert set(state) == {"epoch", "model", "optimizer"} and state["epoch"] == e
        assert len(state["model"]) == 465
        m = TransMVSNet(ndepths=[8, 8, 8])
        m.load_state_dict(state["model"], strict=True)
        adam = torch.optim.Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1.0)
        adam.load_state_dict(state["optimizer"])
        assert float(next(iter(adam.state.values()))["step"]) == 3.0 * (e + 1)
    recs = _records(logdir)
    assert len(recs) == 9
    milestones, gamma = finetune.parse_lrepochs("10,12,14:2", 3)
    for it, r in enumerate(recs):
        assert r["iteration"] == it and r["epoch"] == it // 3 and r["applied"]
        assert r["lr"] == finetune.warmup_multistep_lr(0.001, it, milestones, gamma)
        for k in ("loss", "depth_loss", "epe", "less1", "less3", "step_seconds", "data_wait_seconds"):
            assert np.isfinite(r[k]), (it, k)
    first = np.mean([r["loss"] for r in recs[:3]])
    last = np.mean([r["loss"] for r in recs[6:]])
    print("epoch losses:", [round(float(np.mean([r["loss"] for r in recs[3 * e:3 * e + 3]])), 5) for e in range(3)])
    assert last < first, (first, last)  # the same three samples every epoch


def _ckpt_diff(a, b):
    """(bitwise equal, largest relative difference) over the parameters, buffers and Adam moments."""
    sa, sb = torch.load(a, map_location="cpu"), torch.load(b, map_location="cpu")
    worst, equal = 0.0, True
    pairs = [(sa["model"][k], sb["model"][k]) for k in sa["model"]]
    for i in sa["optimizer"]["state"]:
        for k in ("exp_avg", "exp_avg_sq", "step"):
            pairs.append((sa["optimizer"]["state"][i][k], sb["optimizer"]["state"][i][k]))
    for x, y in pairs:
        equal = equal and torch.equal(x, y)
        x, y = x.double(), y.double()
        worst = max(worst, float((x - y).abs().max() / max(float(y.abs().max()), 1e-30)) if x.numel() else 0.0)
    return equal, worst


def test_driver_resume_is_bitwise(three_epochs, bld_scan, golden_ckpt, tmp_path):
    """Two identical runs end bitwise equal (fixed-order reductions, integer scatter atomics); then one epoch
    plus --resume for the second equals the uninterrupted run bitwise, parameters and Adam moments. (The run
    of three epochs is the first run: its state after epoch 1 does not depend on --epochs.)"""
    root, listfile = bld_scan
    first = os.path.join(three_epochs[0], "model_000001.ckpt")
    again = str(tmp_path / "again")
    finetune.main(_train_args(root, listfile, golden_ckpt, again, 2))
    equal, worst = _ckpt_diff(os.path.join(again, "model_000001.ckpt"), first)
    print("two identical runs: bitwise", equal, "largest relative difference", worst)
    assert equal, worst
    split = str(tmp_path / "split")
    finetune.main(_train_args(root, listfile, golden_ckpt, split, 1))
    assert os.listdir(split).count("model_000000.ckpt") == 1
    res = finetune.main(_train_args(root, listfile, None, split, 2, "--resume"))
    assert res["optimizer"].step_count == 6
    equal, worst = _ckpt_diff(os.path.join(split, "model_000001.ckpt"), first)
    print("one epoch + --resume vs uninterrupted: bitwise", equal, "largest relative difference", worst)
    assert equal, worst
    assert [r["iteration"] for r in _records(split)] == list(range(6))
    assert [r["lr"] for r in _records(split)] == [r["lr"] for r in _records(three_epochs[0])[:6]]


def test_driver_mode_test_dtu(dtu_scan, golden_ckpt, capsys):
    root, listfile = dtu_scan
    res = finetune.main(["--mode", "test", "--dataset", "dtu_yao", "--testpath", root, "--testlist", listfile,
                         "--ndepths", "8,8,8", "--nviews", "3", "--crop", "128,160", "--loadckpt", golden_ckpt])
    m = res["metrics"]
    assert set(ops.EVAL_METRIC_NAMES) <= set(m) and {"loss", "depth_loss", "entropy_loss"} <= set(m)
    assert len(ops.EVAL_METRIC_NAMES) == 12
    for k, v in m.items():
        assert np.isfinite(v), (k, v)
    assert 0 <= m["thres20mm_error"] <= m["thres2mm_error"] <= 1 and m["abs_depth_error"] > 0
    out = capsys.readouterr().out
    assert "final" in out and "abs_depth_error" in out


# ------------------------------------------------------------------ two ranks
def _rank_worker(rank, world, port, argv, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    from transmvsnet_amd import finetune as ft
    saves = []
    save = ft.save_checkpoint
    ft.save_checkpoint = lambda path, *a: (saves.append(path), save(path, *a))
    res = ft.main(argv)
    q.put((rank, res["optimizer"].flat.cpu().numpy().copy(), res["optimizer"].exp_avg.cpu().numpy().copy(), saves))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_driver_two_ranks(golden_ckpt, tmp_path):
    """torch.distributed (env://, nccl), one process per GPU, a 4-view scan: 2 steps per rank. Both ranks end
    with bitwise-equal parameters and only rank 0 writes the checkpoint."""
    import socket

    import torch.multiprocessing as mp
    root = str(tmp_path / "scan")
    listfile = synthetic.write_blended_scan(root, n_views=4, height=128, width=160)
    logdir = str(tmp_path / "log")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    argv = _train_args(root, listfile, golden_ckpt, logdir, 1)
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, argv, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        r, flat, m, saves = q.get(timeout=240)
        res[r] = (flat, m, saves)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert res[0][2] == [os.path.join(logdir, "model_000000.ckpt")] and res[1][2] == []
    assert os.path.exists(os.path.join(logdir, "model_000000.ckpt"))
    assert len(_records(logdir)) == 2
