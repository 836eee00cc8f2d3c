"""Bitwise A/B of every C-ABI launch a test module makes, between two builds of the library (run once per build).

    TMVS_LIB_PATH=variants/X/libtransmvs_hip.so python scripts/diag/launch_bits.py OUT.json tests/test_gpu_X.py [pytest args]
    python scripts/diag/launch_bits.py --compare A.json B.json

Runs the module in-process (pytest.main) with ops._launch wrapped: after each launch, (entry name, sha256 over
every tensor argument -- inputs, outputs and workspaces -- in argument order) is appended to OUT.json. The tests
draw their inputs from fixed seeds, so two builds see the same launches in the same order. --compare prints per
entry how many launches were compared and how many were equal, then a total line; its exit status is 0 only
if everything was compared and equal.
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def compare(path_a, path_b):
    runs = [json.load(open(p)) for p in (path_a, path_b)]
    by_entry = [{}, {}]
    for seen, run in zip(by_entry, runs):
        for name, digest in run:
            seen.setdefault(name, []).append(digest)
    compared = equal = unmatched = 0
    for name in sorted(set(by_entry[0]) | set(by_entry[1])):
        a, b = by_entry[0].get(name, []), by_entry[1].get(name, [])
        n, e = min(len(a), len(b)), sum(x == y for x, y in zip(a, b))
        compared, equal, unmatched = compared + n, equal + e, unmatched + abs(len(a) - len(b))
        print(f"{name:32s} compared {n:5d} equal {e:5d}" + (f"  ({len(a)} against {len(b)} launches)" if len(a) != len(b) else ""))
    ok = compared == equal and not unmatched
    print(f"TOTAL compared {compared} equal {equal} " + ("ALL EQUAL" if ok else "DIFFERENT"))
    return 0 if ok else 1


def record(out_path, pytest_args):
    import pytest
    import torch

    from transmvsnet_amd import ops

    launches = []
    launch = ops._launch

    def recording_launch(name, *args, **kwargs):
        launch(name, *args, **kwargs)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for a in args:
            if isinstance(a, torch.Tensor):
                h.update(a.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
        launches.append((name, h.hexdigest()))

    ops._launch = recording_launch
    try:
        status = int(pytest.main(["-q", "-p", "no:cacheprovider", *pytest_args]))
    finally:
        ops._launch = launch
    with open(out_path, "w") as f:
        json.dump(launches, f)
    print(f"wrote {out_path}: {len(launches)} launches under {os.environ.get('TMVS_LIB_PATH', 'the default library')}, "
          f"pytest status {status}")
    return status


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:4]))
    if len(sys.argv) < 3 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    sys.exit(record(sys.argv[1], sys.argv[2:]))
