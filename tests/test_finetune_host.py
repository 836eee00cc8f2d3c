"""The training driver's host side (transmvsnet_amd.finetune, the training-set readers of
transmvsnet_amd.data, FlatAdam's state_dict) without a GPU, against tests/_train_data_ref.py -- a numpy
restatement of datasets/bld_train.py and datasets/dtu_yao.py -- and against hand values."""
import copy

import numpy as np
import pytest
import torch

from tests import _train_data_ref as ref
from transmvsnet_amd import _lib, build, data, finetune, synthetic
from transmvsnet_amd.train import FlatAdam


@pytest.fixture(scope="module")
def bld_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("bld"))
    return root, synthetic.write_blended_scan(root, n_views=4, height=32, width=48)


@pytest.fixture(scope="module")
def dtu_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dtu"))
    return root, synthetic.write_dtu_train_scan(root, n_views=3, height=16, width=24, margin=(3, 5))


def _same_host_fields(host, proj_ms, want):
    np.testing.assert_array_equal(host["depth_values"], want["depth_values"])
    assert host["depth_values"].dtype == np.float32
    assert host["depth_interval"] == want["depth_interval"]
    for s in ("stage1", "stage2", "stage3"):
        assert proj_ms[s].dtype == np.float32
        np.testing.assert_array_equal(proj_ms[s], want["proj_matrix"][s])


# ------------------------------------------------------------------ readers
def test_bld_reader_matches_restatement(bld_root):
    root, listfile = bld_root
    ds = finetune.BldTrainSet(root, listfile, "train", nviews=3, ndepths=192, device="cpu")
    want = ref.BldRef(root, listfile, 3, 192)
    assert ds.metas == want.metas and len(ds) == len(want) == 4
    for idx in range(len(ds)):
        host, w = ds.load_host(idx), want[idx]
        _same_host_fields(host, ds._stack(host), w)
        # the decoded images: uint8 here, / 255 on the GPU (the float conversion is checked in the GPU tests)
        got = np.stack(host["imgs_u8"]).astype(np.float32) / np.float32(255.)
        np.testing.assert_array_equal(got.transpose(0, 3, 1, 2), w["imgs"])
        np.testing.assert_array_equal(host["depth_raw"], w["depth"]["stage3"])
        # intrinsics / 4, and the interval from the LAST field of line 11: (935 - 425) / 192
        assert host["depth_interval"] == (935.0 - 425.0) / 192
        assert host["depth_end"] == host["depth_interval"] * 191 + 425.0
        assert len(host["depth_values"]) == 192


def test_bld_reader_skips_views_with_too_few_sources(tmp_path):
    root = str(tmp_path)
    listfile = synthetic.write_blended_scan(root, n_views=3, height=16, width=16)
    with open(f"{root}/scan0/cams/pair.txt", "w") as f:  # view 1 has one source only
        f.write("3\n0\n2 1 9.0 2 8.0\n1\n1 0 9.0\n2\n2 0 9.0 1 8.0\n")
    assert [m[1] for m in data.build_list_bld(root, listfile, 3)] == [0, 2]
    assert [m[1] for m in data.build_list_bld(root, listfile, 2)] == [0, 1, 2]
    assert data.build_list_bld(root, listfile, 3) == ref.BldRef(root, listfile, 3).metas
    assert data.build_list_bld(root, listfile, 4) == []


def test_dtu_reader_matches_restatement(dtu_root):
    root, listfile = dtu_root
    ds = finetune.DtuTrainSet(root, listfile, "train", nviews=3, ndepths=192, interval_scale=1.06, device="cpu",
                              target_hw=(16, 24))
    want = ref.DtuRef(root, listfile, 3, 192, 1.06, (16, 24))
    assert ds.metas == want.metas
    assert len(ds) == 3 * 7  # 7 lights per viewpoint
    assert [m[1] for m in ds.metas[:7]] == list(range(7)) and len({m[2] for m in ds.metas[:7]}) == 1
    for idx in (0, 6, 7, 20):
        host, w = ds.load_host(idx), want[idx]
        _same_host_fields(host, ds._stack(host), w)
        assert host["depth_interval"] == 2.5 * 1.06
        got = np.stack(host["imgs_u8"]).astype(np.float32) / np.float32(255.)
        np.testing.assert_array_equal(got.transpose(0, 3, 1, 2), w["imgs"])
    # file ids are vid + 1; the intrinsics are taken as stored (no / 4)
    cams = synthetic.synthetic_cameras(3, 16, 24, seed=1)["stage1"][0].numpy()
    host = ds.load_host(0)
    np.testing.assert_allclose(host["proj"][0][1, :3, :3], cams[0, 1, :3, :3], rtol=1e-6)


def test_image_conversion_is_division_by_255():
    """resize_bilinear at the image's own size (what tmvs_resize_bilinear_u8 restates bitwise) is read_img's
    float32(u8) / 255: every fraction is 0."""
    u8 = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    img = u8.astype(np.float32) / 255.0
    np.testing.assert_array_equal(data.resize_bilinear(img, 16, 16), img)
    for n in (1, 7, 576, 768):
        i0, i1, t = data.resize_axis(n, n)
        assert (i0 == np.arange(n)).all() and (t == 0).all()


def test_nearest_tables():
    """data.nearest_axis is the stated rule; for sizes divisible by the factor it is [::2] / [::4]; the
    composed dtu chain equals resize -> crop -> resize of the restatement."""
    for n_out, n_in in ((18, 37), (9, 37), (25, 50), (12, 50), (35, 71), (46, 93), (64, 128), (144, 576)):
        want = [min(int(np.floor(x * (1.0 / (n_out / n_in)))), n_in - 1) for x in range(n_out)]
        assert data.nearest_axis(n_out, n_in).tolist() == want
    for n in (128, 160, 576, 768, 1200, 1600):
        assert data.nearest_axis(n // 2, n).tolist() == list(range(0, n, 2))
        assert data.nearest_axis(n // 4, n).tolist() == list(range(0, n, 4))
    g = np.random.default_rng(0)
    a = g.random((37, 50)).astype(np.float32)
    np.testing.assert_array_equal(ref.nearest(a, 25, 18), ref.nearest_fast(a, 25, 18))
    np.testing.assert_array_equal(data.resize_nearest(a, 12, 9), ref.nearest(a, 12, 9))
    for (h, w), crop in (((70, 90), (32, 40)), ((71, 93), (32, 40))):
        raw = g.random((h, w)).astype(np.float32)
        rows, cols, hw3 = data.gt_pyramid_tables(h, w, "dtu", crop)
        assert hw3 == crop
        want, _ = ref.gt_pyramid_dtu(raw, np.zeros((h, w), np.uint8), crop)
        r0 = c0 = 0
        for s, k in (("stage3", 1), ("stage2", 2), ("stage1", 4)):
            hs, ws = crop[0] // k, crop[1] // k
            np.testing.assert_array_equal(raw[rows[r0:r0 + hs]][:, cols[c0:c0 + ws]], want[s])
            r0, c0 = r0 + hs, c0 + ws
    rows, cols, _ = data.gt_pyramid_tables(70, 90, "dtu", (32, 40))
    assert (rows[0], cols[0]) == (2 * 1, 2 * 2)  # the crop starts at (1, 2) of the halved image
    with pytest.raises(ValueError):
        data.gt_pyramid_tables(70, 90, "dtu", (36, 40))


# ------------------------------------------------------------------ LR schedule
def test_warmup_multistep_lr_hand_values():
    lr = finetune.warmup_multistep_lr
    base, ms, gamma = 1e-3, [1000, 1200, 1400], 0.5
    assert lr(base, 0, ms, gamma) == base * (1.0 / 3)
    assert lr(base, 250, ms, gamma) == pytest.approx(2 * base / 3, rel=1e-15)
    assert lr(base, 250, ms, gamma) == base * ((1.0 / 3) * 0.5 + 0.5)
    assert lr(base, 499, ms, gamma) < base
    assert lr(base, 500, ms, gamma) == base
    assert lr(base, 999, ms, gamma) == base
    assert lr(base, 1000, ms, gamma) == base * 0.5       # bisect_right: the milestone itself is past
    assert lr(base, 1199, ms, gamma) == base * 0.5
    assert lr(base, 1200, ms, gamma) == base * 0.25
    assert lr(base, 1400, ms, gamma) == lr(base, 10 ** 6, ms, gamma) == base * 0.125
    # a milestone inside the warm-up applies on top of it
    assert lr(base, 250, [100], 0.5) == base * ((1.0 / 3) * 0.5 + 0.5) * 0.5
    # against the reference's formula step by step
    from bisect import bisect_right
    for it in range(0, 1500, 7):
        f = 1
        if it < 500:
            a = float(it) / 500
            f = (1.0 / 3) * (1 - a) + a
        assert lr(base, it, ms, gamma) == base * f * gamma ** bisect_right(ms, it)
    assert finetune.parse_lrepochs("10,12,14:2", 7) == ([70, 84, 98], 0.5)


# ------------------------------------------------------------------ FlatAdam state
def _hand_filled(shapes, step):
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    opt = FlatAdam(ps, lr=2e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=1e-4)
    opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, generator=g))
    opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, generator=g))
    opt._host_steps = step
    opt._step_dev.fill_(step)
    return ps, opt


def test_flat_adam_state_dict_loads_into_torch_adam_and_back():
    shapes = [(8, 1, 3, 3, 3), (16,), (64, 32), ()]
    ps, opt = _hand_filled(shapes, step=3)
    sd = opt.state_dict()
    assert list(sd["state"]) == list(range(len(shapes))) and sd["param_groups"][0]["params"] == list(range(len(shapes)))
    off = 0
    for i, p in enumerate(ps):
        st = sd["state"][i]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3.0
        assert st["exp_avg"].shape == p.shape
        assert torch.equal(st["exp_avg"].reshape(-1), opt.exp_avg[off:off + p.numel()])
        assert torch.equal(st["exp_avg_sq"].reshape(-1), opt.exp_avg_sq[off:off + p.numel()])
        off += p.numel()
    # into torch.optim.Adam over the same shapes, through a file as a checkpoint travels
    tps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    adam = torch.optim.Adam(tps, lr=1.0)
    adam.load_state_dict(copy.deepcopy(sd))  # (torch adopts the tensors it is given; its step writes them)
    g = adam.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (2e-3, (0.8, 0.95), 1e-7, 1e-4)
    for i, p in enumerate(tps):
        assert torch.equal(adam.state[p]["exp_avg"], sd["state"][i]["exp_avg"])
        assert float(adam.state[p]["step"]) == 3.0
    for p in tps:
        p.grad = torch.ones_like(p)
    adam.step()  # the loaded state is usable
    assert float(adam.state[tps[0]]["step"]) == 4.0
    # a torch-made state loads here (int steps as older torch wrote them) and round-trips
    tsd = adam.state_dict()
    for st in tsd["state"].values():
        st["step"] = int(st["step"])
    ps2, opt2 = _hand_filled(shapes, step=0)
    opt2.load_state_dict(tsd)
    assert opt2.step_count == 4 and int(opt2._step_dev.item()) == 4
    assert (opt2.lr, opt2.betas, opt2.eps, opt2.weight_decay) == (2e-3, (0.8, 0.95), 1e-7, 1e-4)
    back = opt2.state_dict()
    for i in range(len(shapes)):
        assert torch.equal(back["state"][i]["exp_avg"], tsd["state"][i]["exp_avg"])
        assert torch.equal(back["state"][i]["exp_avg_sq"], tsd["state"][i]["exp_avg_sq"])
        assert float(back["state"][i]["step"]) == 4.0
    # its own state_dict round-trips bitwise
    ps3, opt3 = _hand_filled(shapes, step=0)
    opt3.load_state_dict(sd)
    assert torch.equal(opt3.exp_avg, opt.exp_avg) and torch.equal(opt3.exp_avg_sq, opt.exp_avg_sq)
    assert opt3.step_count == 3
    # refusals
    with pytest.raises(ValueError):
        FlatAdam([torch.nn.Parameter(torch.zeros(3))]).load_state_dict(sd)
    bad = opt.state_dict()
    bad["state"][1]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError):
        opt3.load_state_dict(bad)
    assert FlatAdam([torch.nn.Parameter(torch.zeros(3))]).state_dict()["state"] == {}


# ------------------------------------------------------------------ parser
def test_parser_defaults_and_checks(capsys):
    a = finetune.parse_args([])
    want = dict(mode="train", dataset="dtu_yao", epochs=16, lr=0.001, lrepochs="10,12,14:2", wd=0.0001, nviews=5,
                batch_size=1, loadckpt=None, logdir="./checkpoints", resume=False, summary_freq=50, save_freq=1,
                eval_freq=1, seed=1, local_rank=0, ndepths="48,32,8", trainpath=None, testpath=None, trainlist=None,
                testlist=None)
    for k, v in want.items():
        assert getattr(a, k) == v, k
    assert (a.interval_scale, a.numdepth, a.loss) == (1.06, 192, "auto")
    with pytest.raises(SystemExit):
        finetune.parse_args(["--resume", "--loadckpt", "x.ckpt"])
    with pytest.raises(SystemExit):
        finetune.parse_args(["--resume", "--mode", "test"])
    assert finetune.parse_args(["--trainpath", "/d"]).testpath == "/d"
    assert finetune.resolve_loss(finetune.parse_args(["--dataset", "bld_train"])) == ("focal_bld", [1.0, 1.0, 1.0])
    assert finetune.resolve_loss(finetune.parse_args(["--dataset", "dtu_yao"])) == ("trans_mvsnet", [0.5, 1.0, 2.0])
    assert finetune.resolve_loss(finetune.parse_args(["--dataset", "dtu_yao", "--loss", "focal_bld"]))[0] == "focal_bld"
    assert finetune.resolve_loss(finetune.parse_args(["--dlossw", "1,2,3"])) == ("trans_mvsnet", [1.0, 2.0, 3.0])
    helptext = finetune.make_parser().format_help()
    for word in ("apex", "tensorboard", "DataParallel"):
        assert word in helptext


def test_epoch_order_and_prefetcher():
    assert finetune.epoch_order(5, 1, 0) == finetune.epoch_order(5, 1, 0)
    assert sorted(finetune.epoch_order(9, 3, 2)) == list(range(9))
    assert finetune.epoch_order(50, 1, 0) != finetune.epoch_order(50, 1, 1)
    g = torch.Generator()
    g.manual_seed(1 + 4)
    assert finetune.epoch_order(9, 1, 4) == torch.randperm(9, generator=g).tolist()

    class _Set:
        def load_host(self, idx):
            return idx

        def upload(self, host):
            return host * 10

    order = [3, 1, 2, 0, 4]
    for workers in (1, 2, 99):
        pf = finetune.Prefetcher(_Set(), order, workers=workers)
        assert pf.workers <= finetune.MAX_WORKERS == 4
        assert list(pf) == [i * 10 for i in order]


# ------------------------------------------------------------------ the two C entries without a GPU
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_new_entries_validate_without_gpu(lib):
    """tmvs_gt_pyramid / tmvs_depth_eval_metrics refuse before any launch (the pointers are host memory that
    is never read; every call has exactly one thing wrong with it)."""
    ARG, SHAPE = -1, -2
    backing = np.zeros(256, np.float32)
    p = (backing.ctypes.data + 63) & ~63
    gp = lib.tmvs_gt_pyramid

    def call(mode=_lib.GT_BLD, depth=p, png=p, h=32, w=40, th=8, tw=12, ptrs=None):
        a = [p] * 8 if ptrs is None else ptrs
        return gp(mode, depth, png, h, w, th, tw, 425.0, 935.0, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], None)

    assert call(depth=None) == ARG
    for nul in range(8):  # rows, cols, the six outputs
        a = [p] * 8
        a[nul] = None
        assert call(ptrs=a) == ARG and call(mode=_lib.GT_DTU, ptrs=a) == ARG, nul
    assert call(mode=_lib.GT_DTU, png=None) == ARG
    assert call(mode=2) == ARG and call(mode=-1) == ARG
    for h, w in ((0, 40), (32, 0), (-1, 40), (32, -1)):
        assert call(h=h, w=w) == SHAPE and call(mode=_lib.GT_DTU, h=h, w=w) == SHAPE, (h, w)
    for th, tw in ((0, 12), (8, 0), (-8, 12), (17, 12), (8, 21), (16, 21)):  # the halved image is 16 x 20
        assert call(mode=_lib.GT_DTU, th=th, tw=tw) == SHAPE, (th, tw)
    assert call(h=3, w=40) == SHAPE and call(mode=_lib.GT_DTU, th=3) == SHAPE  # an empty stage 1

    em = lib.tmvs_depth_eval_metrics
    need = lib.tmvs_depth_eval_metrics_workspace(16)
    assert need == 1024 * (7 * 8 + 12 * 4)
    big = 1 << 40
    for nul in range(5):
        a = [p] * 5
        a[nul] = None
        assert em(a[0], a[1], a[2], 16, a[3], big, a[4], None) == ARG, nul
    for n in (0, -1):
        assert em(p, p, p, n, p, big, p, None) == ARG
    assert em(p, p, p, 16, p, need - 1, p, None) == ARG
    assert em(p, p, p, 16, p + 4, big, p, None) == ARG  # the fp64 partials need 8-byte alignment
