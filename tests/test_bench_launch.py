"""bench.py's launcher logic (CPU): how `--gpus N` maps onto rank processes, without a GPU."""
import pytest

import bench


def test_single_process_default():
    assert bench.resolve_launch(1, {}) == ("rank", 1, 0, 0)


def test_gpus_n_without_launcher_spawns():
    assert bench.resolve_launch(8, {}) == ("spawn", 8)
    assert bench.resolve_launch(2, {"MASTER_ADDR": "127.0.0.1"}) == ("spawn", 2)


def test_torchrun_env_is_one_rank():
    env = {"WORLD_SIZE": "4", "RANK": "2", "LOCAL_RANK": "2"}
    assert bench.resolve_launch(4, env) == ("rank", 4, 2, 2)
    # `--gpus` left at its default under torchrun: the env decides
    assert bench.resolve_launch(1, env) == ("rank", 4, 2, 2)


def test_mismatched_world_refused():
    with pytest.raises(SystemExit):
        bench.resolve_launch(8, {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    with pytest.raises(SystemExit):
        bench.resolve_launch(0, {})


def test_spawned_rank_env_round_trips():
    for r in range(3):
        env = bench.rank_env(r, 3, 29555)
        assert env["MASTER_ADDR"] == "127.0.0.1" and env["MASTER_PORT"] == "29555"
        assert bench.resolve_launch(3, env) == ("rank", 3, r, r)


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench._args()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench._args()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_writes_every_array_and_samples_large_ones(tmp_path, monkeypatch):
    import json
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    g = torch.Generator().manual_seed(0)

    def stage(d, h, w):
        return {"depth": torch.rand(1, h, w, generator=g), "photo_confidence": torch.rand(1, h, w, generator=g),
                "prob_volume": torch.rand(1, d, h, w, generator=g), "depth_values": torch.rand(1, d, h, w, generator=g)}

    out = {"stage1": stage(4, 3, 5), "stage2": stage(3, 6, 10), "stage3": stage(2, 12, 20)}
    out.update(out["stage3"])  # forward_features' layout: the last stage's entries at top level too
    bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    names = [f"{p}{k}" for p in ("", "stage1_", "stage2_") for k in out["stage3"]]
    man = json.load(open(tmp_path / "a" / "manifest.json"))["arrays"]
    assert sorted(man) == sorted(names)
    for n in names:
        a, b = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        src = out[n] if n in out else out[n[:6]][n[7:]]
        assert a.dtype == np.float32 and np.array_equal(a, b)
        assert man[n]["shape"] == list(src.shape) and man[n]["sampled"] == (src.numel() > 100)
        if man[n]["sampled"]:  # a fixed sample of the flattened array: sorted, distinct indices
            assert a.shape == (100,)
            idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(src.numel(), 100, replace=False))
            assert np.array_equal(a, src.reshape(-1).numpy()[idx])
        else:
            assert np.array_equal(a, src.numpy())


def test_host_cores_reports_affinity():
    import os
    n, quota, model = bench.host_cores()
    assert n == len(os.sched_getaffinity(0)) and isinstance(model, str)
    assert quota is None or quota > 0
