"""tmvs_dynamic_fusion at the C4 (Tanks & Temples) size: one reference view of 1056x1920 with 10 source
views (synthetic plane scene, tests/_dynfusion_scene.py). 3 warm-ups, then the median of 20 HIP-event
timings of the launch; the CPU restatement (tests/_dynfusion_ref.py, numpy) on the same input for scale;
the compulsory bytes per view H*W*(4 + 4*S + 4 + 1 + 1 + 4 + 12) -- own depth, one texel per source,
confidence, the four outputs -- and the GB/s they give. A record, not a test.
Usage: dynamic_fusion_time.py [--out profiles/dynamic_fusion_time.json] [--no-cpu]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from tests import _dynfusion_ref as ref
from tests._dynfusion_scene import make_scene
from transmvsnet_amd import dynamic_fusion as dynf

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/dynamic_fusion_time.json"
V, H, W, S = 11, 1056, 1920, 10
PHOTO, THRES = 0.18, 5  # scripts/test_tnt.sh
t0 = time.time()
d, c, _, ks, es = make_scene(V, H, W, seed=1)
print(f"scene {V}x{H}x{W} built in {time.time() - t0:.1f} s", flush=True)
srcs = list(range(1, V))
dd, cd = torch.from_numpy(d).cuda(), torch.from_numpy(c[0]).cuda()
consts = dynf.view_constants(ks, es, 0, srcs, dd.device)
out = dynf.alloc_outputs(H, W, dd.device)
res = {}
for bits in (5, 0):
    ts = []
    for rep in range(23):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = dynf.filter_view(dd, cd, ks, es, 0, srcs, PHOTO, THRES, bits, consts=consts, out=out)
        e1.record()
        torch.cuda.synchronize()
        if rep >= 3:
            ts.append(e0.elapsed_time(e1))
    res[bits] = (float(np.median(ts)), float(np.min(ts)), r["geo"].float().mean().item(),
                 r["final"].float().mean().item())
    print(f"subpixel_bits={bits}: median {res[bits][0] * 1e3:.1f} us, min {res[bits][1] * 1e3:.1f} us; "
          f"geo {res[bits][2]:.3f}, final {res[bits][3]:.3f}", flush=True)
cpu_s = None
if "--no-cpu" not in sys.argv:
    t0 = time.perf_counter()
    want = ref.filter_view_ref(d, c[0], ks, es, 0, srcs, PHOTO, THRES, 5)
    cpu_s = time.perf_counter() - t0
    got = dynf.filter_view(dd, cd, ks, es, 0, srcs, PHOTO, THRES, 5, consts=consts, out=out)
    ok = ~want["ambiguous"]
    mism = int(((got["final"].cpu().numpy() != want["final"]) & ok).sum())
    print(f"CPU restatement {cpu_s:.2f} s; final-mask mismatches outside {int((~ok).sum())} ambiguous pixels: {mism}")
nbytes = H * W * (4 + 4 * S + 4 + 1 + 1 + 4 + 12)
rec = {"workload": f"one reference view {H}x{W}, {S} sources, photo_threshold {PHOTO}, thres_view {THRES}",
       "kernel_ms_median_of_20": res[5][0], "kernel_ms_min": res[5][1],
       "kernel_ms_median_subpixel_bits_0": res[0][0], "geo_fraction": res[5][2], "final_fraction": res[5][3],
       "cpu_restatement_s": cpu_s, "speedup_vs_cpu_restatement": None if cpu_s is None else cpu_s * 1e3 / res[5][0],
       "compulsory_bytes_per_view": nbytes, "compulsory_gb_per_s": nbytes / (res[5][0] * 1e-3) / 1e9}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
