"""The scene reconstruction driver on the GPU: tmvs_depth_postprocess and tmvs_resize_bilinear_u8 / _f32
against the host functions they replace (tests/_postprocess_ref.py, data.resize_bilinear), ViewCache's
samples against data.load_sample / load_sample_tnt, and reconstruct_scan end to end, with planted geometry
behind a stub model (both datasets, in-memory cloud vs the cloud of the written files) and with the real
TransMVSNet. Every comparison is exact: the kernels restate float32 / float64 arithmetic that numpy
performs deterministically, so there is no tolerance to choose."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _postprocess_ref as ref
from tests._util import golden_state_dict
from tests.test_data_io import _write_scan
from tests.test_reconstruct import _dtu_scan
from transmvsnet_amd import TransMVSNet, data, fusion, reconstruct
from transmvsnet_amd import dynamic_fusion as dynf

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(4, 4), (8, 12), (36, 52), (96, 128)]


@functools.lru_cache(maxsize=None)
def _case(h, w):
    inputs = ref.seeded_inputs(h, w)
    return inputs, ref.postprocess_ref(*inputs), ref.postprocess_ref(*inputs[:4])


def _outputs(depth, conf3, conf2, conf1):
    up = lambda a: torch.from_numpy(a).to(DEV)[None]
    return {"depth": up(depth), "photo_confidence": up(conf3), "stage1": {"photo_confidence": up(conf1)},
            "stage2": {"photo_confidence": up(conf2)}}


def _equal(got, want, tag):
    assert set(got) == set(want), tag
    for k in want:
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (tag, k)
        np.testing.assert_array_equal(g, want[k], err_msg=f"{tag} {k}")


# ------------------------------------------------------------------ tmvs_depth_postprocess
@pytest.mark.parametrize("shape", SHAPES)
def test_depth_postprocess_vs_restatement(shape):
    """4 x 4: conf1 is 1 x 1, every tap clamps; 36 x 52: the block tail falls in both axes."""
    h, w = shape
    inputs, want, want_noimg = _case(h, w)
    outs = _outputs(*inputs[:4])
    image = torch.from_numpy(inputs[4]).to(DEV)
    _equal(reconstruct.postprocess_view(outs, image), want, (shape, "image"))
    _equal(reconstruct.postprocess_view(outs), want_noimg, (shape, "no image"))
    # into slots of slabs, as the driver calls it; the neighbouring slots stay untouched
    slab = {"conf_final": torch.full((3, h, w), -1.0, device=DEV), "depth": torch.full((3, h, w), -1.0, device=DEV),
            "rgbd": torch.full((3, h, w, 4), -1.0, device=DEV)}
    rgba = torch.zeros(h, w, 4, dtype=torch.uint8, device=DEV)
    got = reconstruct.postprocess_view(outs, image, out={"conf_final": slab["conf_final"][1], "depth": slab["depth"][1],
                                                         "rgbd": slab["rgbd"][1], "rgba_u8": rgba})
    _equal(got, want, (shape, "slab"))
    assert got["rgbd"].data_ptr() == slab["rgbd"][1].data_ptr()
    for t in slab.values():
        assert bool((t[0] == -1).all()) and bool((t[2] == -1).all())


def test_depth_postprocess_other_threshold_and_range():
    h, w = 36, 52
    inputs, _, _ = _case(h, w)
    want = ref.postprocess_ref(*inputs, conf_threshold=0.05, depth_min=400.0, depth_max=1000.0)
    got = reconstruct.postprocess_view(_outputs(*inputs[:4]), torch.from_numpy(inputs[4]).to(DEV), 0.05, 400.0, 1000.0)
    for k in ("conf_final", "depth", "rgba_u8"):
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k], err_msg=k)
    # the (B, G, R) texels do not depend on the range; the decode keeps fusibile's 425 + 512 a
    np.testing.assert_array_equal(got["rgbd"].cpu().numpy(),
                                  fusion.rgbd_from_images(want["rgba_u8"][..., [2, 1, 0]], want["rgba_u8"][..., 3]))


def test_depth_postprocess_wrapper_checks():
    inputs, _, _ = _case(8, 12)
    outs = _outputs(*inputs[:4])
    image = torch.from_numpy(inputs[4]).to(DEV)
    with pytest.raises(ValueError):
        reconstruct.postprocess_view(outs, image[:, :4].contiguous())
    with pytest.raises(ValueError):
        reconstruct.postprocess_view(dict(outs, stage1={"photo_confidence": outs["stage2"]["photo_confidence"]}))
    with pytest.raises(ValueError):
        reconstruct.postprocess_view(outs, out={"rgbd": torch.empty(8, 12, 4, device=DEV)})
    with pytest.raises(RuntimeError):
        reconstruct.postprocess_view(dict(outs, depth=outs["depth"].double()))
    with pytest.raises(ValueError):
        reconstruct.postprocess_view({k: (v[:, :6] if k == "depth" else v) for k, v in outs.items()})


def test_depth_postprocess_graph_capture():
    """One captured-and-replayed launch equals the eager one: no allocation, no synchronisation."""
    h, w = 36, 52
    inputs, want, _ = _case(h, w)
    outs = _outputs(*inputs[:4])
    image = torch.from_numpy(inputs[4]).to(DEV)
    eager = {k: t.clone() for k, t in reconstruct.postprocess_view(outs, image).items()}
    out = reconstruct.alloc_outputs(h, w, DEV)
    for t in out.values():
        t.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = reconstruct.postprocess_view(outs, image, out=out)
    for t in out.values():
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    _equal(res, want, "replayed")
    for k in eager:
        assert res[k].data_ptr() == out[k].data_ptr()
        np.testing.assert_array_equal(res[k].cpu().numpy(), eager[k].cpu().numpy(), err_msg=k)


# ------------------------------------------------------------------ the resize
@pytest.mark.parametrize("sizes", [((30, 40), (19, 27)), ((13, 17), (32, 48)), ((300, 400), (288, 384)),
                                   ((30, 40), (30, 40))])
def test_resize_bilinear_u8_vs_host(sizes, tmp_path):
    """read_img + resize_bilinear + the CHW transpose: down, up, the scan size of the data tests, identity."""
    from PIL import Image
    (h, w), (nh, nw) = sizes
    src = np.random.default_rng(h + nw).integers(0, 256, (h, w, 3), dtype=np.uint8)
    src[0, 0], src[-1, -1] = 255, 0
    fn = str(tmp_path / "img.png")
    Image.fromarray(src).save(fn)
    np.testing.assert_array_equal(reconstruct.read_img_u8(fn), src)
    want = data.resize_bilinear(data.read_img(fn), nw, nh).transpose(2, 0, 1)
    got = reconstruct.resize_image(torch.from_numpy(src).to(DEV), nw, nh)
    assert got.shape == (3, nh, nw) and got.dtype == torch.float32 and got.is_contiguous()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    if (h, w) == (nh, nw):
        np.testing.assert_array_equal(got.cpu().numpy(), (src.astype(np.float32) / 255.0).transpose(2, 0, 1))


def test_resize_bilinear_f32_vs_host():
    """The second resize of an already loaded image (float32 CHW in and out)."""
    img = np.random.default_rng(5).random((37, 45, 3)).astype(np.float32)
    chw = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).to(DEV)
    for nh, nw in ((64, 96), (20, 31)):
        got = reconstruct.resize_image(chw, nw, nh)
        np.testing.assert_array_equal(got.cpu().numpy(), data.resize_bilinear(img, nw, nh).transpose(2, 0, 1))


# ------------------------------------------------------------------ ViewCache
def _same_sample(got, want):
    np.testing.assert_array_equal(got["imgs"].cpu().numpy(), want["imgs"])
    for k in ("stage1", "stage2", "stage3"):
        np.testing.assert_array_equal(got["proj_matrix"][k], want["proj_matrix"][k])
    np.testing.assert_array_equal(got["depth_values"], want["depth_values"])


@pytest.mark.parametrize("cap", [(864, 1152), (216, 288)])
def test_view_cache_samples_equal_load_sample(tmp_path, cap):
    """300 x 400 with no rescale, and a cap that rescales plus a view of another size (the second resize);
    every JPEG is decoded once however many samples use it."""
    metas = _dtu_scan(tmp_path)
    max_h, max_w = cap
    cache = reconstruct.ViewCache(str(tmp_path), "scan1", "dtu", DEV, nviews=4, max_h=max_h, max_w=max_w)
    for ref_view, srcs in metas:
        want = data.load_sample(str(tmp_path), "scan1", ref_view, srcs, nviews=4, max_h=max_h, max_w=max_w)
        _same_sample(cache.sample(ref_view, srcs), want)
    assert cache.decoded == 4


def test_view_cache_samples_equal_load_sample_tnt(tmp_path):
    td = str(tmp_path)
    _write_scan(td, "Family", 4, "cams_1", tnt=True)
    metas = data.read_pair_file(os.path.join(td, "Family", "pair.txt"), pad=False)
    cache = reconstruct.ViewCache(td, "Family", "tnt", DEV)
    want = data.load_sample_tnt(td, "Family", metas[0][0], metas[0][1], nviews=11)
    _same_sample(cache.sample(*metas[0]), want)
    cache2 = reconstruct.ViewCache(td, "Family", "tnt", DEV, image_size=(256, 192), fixed_hw=cache.fixed_hw)
    want2 = data.load_sample_tnt(td, "Family", 1, [0, 2], image_size=(256, 192), fixed_hw=want["fixed_hw"])
    got2 = cache2.sample(1, [0, 2])
    assert got2["imgs"].shape == (3, 3, 288, 384)
    _same_sample(got2, want2)


# ------------------------------------------------------------------ end to end, planted geometry
def test_reconstruct_dtu_planted(tmp_path):
    """The in-memory cloud equals the cloud of the --save_outputs files (camera/*.txt through fusibile's
    reader, image/*.png through its decode), coordinates and textures both, and is not empty."""
    sc = ref.planted_scene()
    v, (h, w) = len(sc["depths"]), sc["depths"].shape[1:]
    root, out = str(tmp_path / "in"), str(tmp_path / "out")
    ref.write_planted_scan(root, "scan1", sc, "cams")
    model = ref.StubModel(sc, DEV)
    res = reconstruct.reconstruct_scan(model, root, "scan1", "dtu", out, save_outputs=True)
    assert [i for i, _ in model.calls] == list(range(v)) and model.calls[0][1] == (1, 5, 3, h, w)
    assert res["views"] == list(range(v)) and res["decoded"] == v
    assert res["ply"] == os.path.join(out, "scan1", "3d_model.ply")
    # per view: the slabs hold the restatement of the planted outputs on the image the driver loaded
    packs, bgr, alpha = [], [], []
    for i in range(v):
        img = data.read_img(os.path.join(root, "scan1", "images", "{:0>8}.jpg".format(i))).transpose(2, 0, 1)
        want = ref.postprocess_ref(sc["depths"][i], sc["conf3"][i], sc["conf2"][i], sc["conf1"][i], img)
        np.testing.assert_array_equal(res["depth"][i].cpu().numpy(), want["depth"])
        np.testing.assert_array_equal(res["conf"][i].cpu().numpy(), want["conf_final"])
        np.testing.assert_array_equal(res["rgbd"][i].cpu().numpy(), want["rgbd"])
        b, a = reconstruct.read_rgba_png(os.path.join(out, "scan1", "image", "{:0>8}.png".format(i)))
        np.testing.assert_array_equal(np.concatenate([b[..., ::-1], a[..., None]], 2), want["rgba_u8"])
        bgr.append(b)
        alpha.append(a)
        packs.append(fusion.camera_params(fusion.read_cam(os.path.join(out, "scan1", "camera", "{:0>8}.txt".format(i))))[0])
    np.testing.assert_array_equal(np.stack(packs), res["cams_packed"])
    rgbd = fusion.rgbd_from_images(np.stack(bgr), np.stack(alpha))
    xs, ts = fusion.fuse(torch.from_numpy(rgbd).to(DEV), np.stack(packs))
    print("dtu planted: fused points", len(xs), "of", v * h * w)
    assert len(xs) > 0.2 * h * w
    assert torch.equal(res["points"], xs) and torch.equal(res["textures"], ts)
    head, body = open(res["ply"], "rb").read().split(b"end_header\n")
    assert ("element vertex %d\n" % len(xs)).encode() in head and len(body) == 15 * len(xs)


def test_reconstruct_tnt_planted(tmp_path):
    """In-memory points equal dynamic_fusion.fuse_scan on the written folder, in the same order; the
    colours are compared within the in-memory path (the written JPEG is lossy)."""
    sc = ref.planted_scene()
    v, (h, w) = len(sc["depths"]), sc["depths"].shape[1:]
    root, out = str(tmp_path / "in"), str(tmp_path / "out")
    ref.write_planted_scan(root, "Family", sc, "cams_1")
    model = ref.StubModel(sc, DEV)
    res = reconstruct.reconstruct_scan(model, root, "Family", "tnt", out, photo_threshold=0.3, thres_view=3,
                                       save_outputs=True)
    assert [i for i, _ in model.calls] == list(range(v)) and res["fixed_hw"] == (h, w) and res["decoded"] == v
    assert res["ply"] == os.path.join(out, "Family.ply")
    pts, _ = dynf.fuse_scan(os.path.join(out, "Family"), os.path.join(root, "Family", "pair.txt"),
                            str(tmp_path / "from_files.ply"), None, 0.3, 3)
    print("tnt planted: fused points", len(pts), "of", v * h * w)
    assert len(pts) > 0.1 * v * h * w
    assert torch.equal(res["points"], pts)
    # colours: (image * 255) truncated, of the images the driver loaded, where the final mask is set
    cols = []
    for i in range(v):
        img = torch.from_numpy(data.read_img(os.path.join(root, "Family", "images", "{:0>8}.jpg".format(i)))).to(DEV)
        r = dynf.filter_view(res["depth"], res["conf"][i], res["Ks"], res["Es"], *res["pairs"][i], 0.3, 3)
        cols.append((img[r["final"]] * 255).to(torch.uint8))
    assert torch.equal(res["colors"], torch.cat(cols))
    rec = np.frombuffer(open(res["ply"], "rb").read().split(b"end_header\n")[1],
                        dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    np.testing.assert_array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), pts.cpu().numpy())
    # the written depth and confidence maps are the slabs, and the images are at the depth maps' size
    d0, _ = data.read_pfm(os.path.join(out, "Family", "depth_est", "{:0>8}.pfm".format(2)))
    np.testing.assert_array_equal(d0, res["depth"][2].cpu().numpy())
    assert data.read_img(os.path.join(out, "Family", "images", "{:0>8}.jpg".format(2))).shape == (h, w, 3)


# ------------------------------------------------------------------ end to end, the real network
def test_reconstruct_real_model(tmp_path):
    """A 288 x 384 scan of 3 reference views through TransMVSNet: per view the driver's conf_final and
    depth equal the restatement applied to a plain model(...) call on data.load_sample's arrays; the PLY
    exists and parses."""
    td, out = str(tmp_path / "in"), str(tmp_path / "out")
    _write_scan(td, "scan1", 3, "cams", h=300, w=400, seed=8)
    m = TransMVSNet(ndepths=[48, 32, 8]).eval()
    m.load_state_dict(golden_state_dict(), strict=True)
    m = m.to(DEV)
    seen = {}

    def on_view(slot, ref_view, sample, post):
        seen[ref_view] = {k: post[k].clone() for k in ("conf_final", "depth")}

    res = reconstruct.reconstruct_scan(m, td, "scan1", "dtu", out, nviews=3, on_view=on_view)
    assert res["views"] == [0, 1, 2] and res["decoded"] == 3 and tuple(res["depth"].shape) == (3, 288, 384)
    metas = data.read_pair_file(os.path.join(td, "scan1", "pair.txt"), nviews=3)
    for ref_view, srcs in metas:
        s = data.load_sample(td, "scan1", ref_view, srcs, nviews=3)
        with torch.no_grad():
            o = m(torch.from_numpy(s["imgs"])[None].to(DEV), {k: torch.from_numpy(p)[None] for k, p in
                                                              s["proj_matrix"].items()},
                  torch.from_numpy(s["depth_values"])[None].to(DEV))
        npy = lambda t: t[0].cpu().numpy()
        want = ref.postprocess_ref(npy(o["depth"]), npy(o["photo_confidence"]), npy(o["stage2"]["photo_confidence"]),
                                   npy(o["stage1"]["photo_confidence"]))
        np.testing.assert_array_equal(seen[ref_view]["conf_final"].cpu().numpy(), want["conf_final"])
        np.testing.assert_array_equal(seen[ref_view]["depth"].cpu().numpy(), want["depth"])
    head, body = open(res["ply"], "rb").read().split(b"end_header\n", 1)
    n = int([ln for ln in head.decode().split("\n") if ln.startswith("element vertex")][0].split()[2])
    assert n == len(res["points"]) and len(body) == 15 * n
