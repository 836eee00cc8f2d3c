"""What the reconstruction driver's stages cost per reference view at the C2 size (DTU: source images
1200x1600 resized to 864x1152, N = 5 views per forward), next to the forward:

  host input      data.read_img + data.scale_mvs_input for the N images of one sample (what load_sample does
                  for every sample), split into the JPEG decode and the numpy resize
  GPU input       the decode (unchanged), then upload of the uint8 image + tmvs_resize_bilinear_u8, per image;
                  ViewCache runs it once per view of the scan instead of N times per reference view
  forward         TransMVSNet.forward, B = 1, N = 5, synthetic weights
  postprocess     one tmvs_depth_postprocess launch with image, rgba_u8 and rgbd (HIP events around
                  REPS back-to-back launches), and the bytes the algorithm has to move: per pixel 4 + 4 + 1 +
                  0.25 + 12 read (depth, conf3, conf2 / 4, conf1 / 16, image) and 4 + 4 + 4 + 16 written
  numpy           the composition it replaces (tests/_postprocess_ref.py: resize_bilinear x 2, product, mask,
                  depth_normal, clip, rgbd_from_images) plus the device -> host copies of its four inputs

Host clocks surround work that ends in a device synchronise; medians over the repetitions after warm-ups.
A record, not a test. Usage: reconstruct_time.py [--out profiles/reconstruct_time.json] [--no-forward]"""
import json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from tests import _postprocess_ref as ref
from transmvsnet_amd import TransMVSNet, data, reconstruct, synthetic

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/reconstruct_time.json"
SRC_H, SRC_W, H, W, N = 1200, 1600, 864, 1152, 5
REPS = 200
assert torch.cuda.is_available(), "reconstruct_time.py measures on the GPU"
dev = torch.device("cuda")
med = lambda ts: float(np.median(ts))


def clock(fn, reps, warm=2):
    ts = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return med(ts), float(np.min(ts))


rec = {"workload": f"one reference view, source {SRC_H}x{SRC_W} -> {H}x{W}, N = {N}"}
with tempfile.TemporaryDirectory() as td:
    from PIL import Image
    rng = np.random.default_rng(0)
    ys, xs = np.mgrid[0:SRC_H, 0:SRC_W]
    img = np.stack([127 + 100 * np.sin(xs / 37.0 + ys / 91.0), 127 + 100 * np.cos(xs / 53.0), 127 + 100 * np.sin(ys / 29.0)], -1)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    fn = os.path.join(td, "00000000.jpg")
    Image.fromarray(img).save(fn, quality=95)
    k = np.float32([[2892.33 / 4, 0, 823.205 / 4], [0, 2883.18 / 4, 619.071 / 4], [0, 0, 1]])
    # host path
    rec["host_decode_ms_per_image"] = clock(lambda: data.read_img(fn), 5, 1)[0]
    f32 = data.read_img(fn)
    rec["host_resize_ms_per_image"] = clock(lambda: data.scale_mvs_input(f32, k, W, H), 5, 1)[0]
    rec["host_input_ms_per_reference_view"] = clock(
        lambda: [data.scale_mvs_input(data.read_img(fn), k, W, H) for _ in range(N)], 3, 1)[0]
    # GPU path
    tables = reconstruct._AxisTables(dev)
    u8 = reconstruct.read_img_u8(fn)
    rec["u8_decode_ms_per_image"] = clock(lambda: reconstruct.read_img_u8(fn), 5, 1)[0]
    rec["gpu_upload_resize_ms_per_image"] = clock(
        lambda: reconstruct.resize_image(torch.from_numpy(u8).to(dev), W, H, tables), 20, 3)[0]
    src_d = torch.from_numpy(u8).to(dev)
    rec["gpu_resize_kernel_ms"] = clock(lambda: reconstruct.resize_image(src_d, W, H, tables), 50, 3)[0]
    got = reconstruct.resize_image(src_d, W, H, tables).cpu().numpy()
    rec["gpu_resize_equals_host"] = bool(np.array_equal(got, data.scale_mvs_input(f32, k, W, H)[0].transpose(2, 0, 1)))
    rec["gpu_input_ms_per_image_decode_included"] = rec["u8_decode_ms_per_image"] + rec["gpu_upload_resize_ms_per_image"]
    print(json.dumps(rec), flush=True)

# postprocess
depth, conf3, conf2, conf1, image = ref.seeded_inputs(H, W)
up = lambda a: torch.from_numpy(a).to(dev)[None]
outs = {"depth": up(depth), "photo_confidence": up(conf3), "stage1": {"photo_confidence": up(conf1)},
        "stage2": {"photo_confidence": up(conf2)}}
image_d = torch.from_numpy(image).to(dev)
out = reconstruct.alloc_outputs(H, W, dev)
for _ in range(5):
    reconstruct.postprocess_view(outs, image_d, out=out)
ts = []
for _ in range(7):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        reconstruct.postprocess_view(outs, image_d, out=out)
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1) / REPS)
nbytes = H * W * (4 + 4 + 1 + 0.25 + 12 + 4 + 4 + 4 + 16)
rec["postprocess_ms_per_launch_back_to_back"] = med(ts)
rec["postprocess_ms_single_call_synchronised"] = clock(lambda: reconstruct.postprocess_view(outs, image_d, out=out), 50, 3)[0]
rec["postprocess_algorithmic_bytes"] = nbytes
rec["postprocess_gb_per_s"] = nbytes / (med(ts) * 1e-3) / 1e9


def numpy_path():
    n = lambda t: t[0].cpu().numpy()
    return ref.postprocess_ref(n(outs["depth"]), n(outs["photo_confidence"]), n(outs["stage2"]["photo_confidence"]),
                               n(outs["stage1"]["photo_confidence"]), image)


rec["numpy_composition_ms_with_d2h"] = clock(numpy_path, 5, 1)[0]
want = numpy_path()
rec["postprocess_equals_numpy"] = all(np.array_equal(out[k].cpu().numpy(), want[k], equal_nan=k == "conf_final")
                                      for k in want)
print(json.dumps(rec), flush=True)

if "--no-forward" not in sys.argv:
    m = TransMVSNet().eval()
    m.load_state_dict(synthetic.synthetic_state_dict(synthetic.state_dict_shapes(m), seed=0, sharpen=100.0), strict=True)
    m = m.to(dev)
    imgs = synthetic.synthetic_images(N, H, W, seed=0).to(dev)
    proj = synthetic.synthetic_cameras(N, H, W, seed=1)
    dv = synthetic.synthetic_depth_values(1).to(dev)
    with torch.no_grad():
        rec["forward_ms"] = clock(lambda: m(imgs, proj, dv), 10, 3)[0]

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
