"""The training driver's batching without a GPU: --batch_size on the command line, the refusal of focal_bld
on a batch (BlendedMVS fine-tuning is batch 1 in the reference), how an epoch's order is cut into batches
(the reference's train loader drops the remainder, its test loader keeps a smaller last batch), and the
iterations per epoch that the LR milestones and --resume count in."""
import numpy as np
import pytest
import torch

from transmvsnet_amd import finetune, loss


def test_parser_accepts_a_batch_size():
    assert finetune.parse_args([]).batch_size == 1
    args = finetune.parse_args(["--batch_size", "2"])
    assert args.batch_size == 2 and args.dataset == "dtu_yao"
    assert finetune.resolve_loss(args) == ("trans_mvsnet", [0.5, 1.0, 2.0])
    assert finetune.parse_args(["--batch_size", "5", "--dataset", "bld_train", "--loss", "trans_mvsnet"]).batch_size == 5
    assert finetune.parse_args(["--batch_size", "1", "--dataset", "bld_train"]).batch_size == 1
    for bad in ("0", "-1"):
        with pytest.raises(SystemExit):
            finetune.parse_args(["--batch_size", bad])
    assert "batch" in finetune.make_parser().description and "one sample per rank" not in \
        " ".join(finetune.make_parser().description.split())


@pytest.mark.parametrize("argv", [["--batch_size", "2", "--dataset", "bld_train"],
                                  ["--batch_size", "3", "--loss", "focal_bld"]])
def test_focal_bld_on_a_batch_is_refused_when_the_arguments_are_parsed(argv, capsys):
    with pytest.raises(SystemExit) as e:
        finetune.parse_args(argv)
    assert e.value.code == 2
    err = " ".join(capsys.readouterr().err.split())
    assert "BlendedMVS fine-tuning is batch 1 in the reference" in err and "trans_mvsnet" in err and "dtu_yao" in err
    assert "BlendedMVS fine-tuning is batch 1 in the reference" in loss.FOCAL_BLD_BATCH_MSG


def test_focal_loss_bld_says_why_it_refuses_a_batch_of_intervals():
    with pytest.raises(ValueError, match="BlendedMVS fine-tuning is batch 1 in the reference"):
        loss.focal_loss_bld({}, {}, {}, torch.tensor([2.5, 2.5]))


def test_batches_of_an_order():
    order = [5, 3, 6, 0, 2, 4, 1]
    train = finetune.batches(order, 2, drop_last=True)
    test = finetune.batches(order, 2, drop_last=False)
    assert train == [[5, 3], [6, 0], [2, 4]]            # 7 samples at B = 2: 3 training batches, sample 1 dropped
    assert test == [[5, 3], [6, 0], [2, 4], [1]]        # 4 evaluation batches, the last of one sample
    assert finetune.batches(order, 1, True) == finetune.batches(order, 1, False) == [[i] for i in order]
    assert finetune.batches(order, 7, True) == [order] and finetune.batches(order, 8, True) == []
    assert finetune.batches(order, 8, False) == [order] and finetune.batches([], 2, False) == []
    for n in range(0, 12):
        for b in (1, 2, 3, 5):
            got = finetune.batches(range(n), b, True)
            assert len(got) == n // b == finetune.iters_per_epoch(n, b) and all(len(g) == b for g in got)
            kept = finetune.batches(range(n), b, False)
            assert len(kept) == -(-n // b) and [i for g in kept for i in g] == list(range(n))
    with pytest.raises(ValueError):
        finetune.batches(order, 0, True)


def test_iterations_per_epoch_feed_the_lr_milestones():
    """27 samples on this rank: 27 iterations per epoch at B = 1, 13 at B = 2 -- the milestones, the warm-up
    and the first iteration after a resume are counted in those."""
    assert finetune.iters_per_epoch(27, 1) == 27 and finetune.iters_per_epoch(27, 2) == 13
    ms, gamma = finetune.parse_lrepochs("10,12,14:2", finetune.iters_per_epoch(27, 2))
    assert ms == [130, 156, 182] and gamma == 0.5
    lr = [finetune.warmup_multistep_lr(1e-3, it, ms, gamma, warmup_iters=0) for it in (129, 130, 155, 156, 182)]
    assert lr == [1e-3, 5e-4, 5e-4, 2.5e-4, 1.25e-4]
    assert finetune.iters_per_epoch(27, 2) * 3 == 39  # --resume after epoch 2 starts at iteration 39


def test_batch_loader_groups_what_the_prefetcher_yields():
    class Set:
        def load_host(self, idx):
            return idx

        def upload(self, host):
            return {"idx": host}

    loader = finetune.BatchLoader(Set(), [[4, 1], [3, 0], [2]], workers=2)
    assert len(loader) == 3
    assert [[s["idx"] for s in group] for group in loader] == [[4, 1], [3, 0], [2]]
    assert loader.wait_s >= 0.0
    assert [len(g) for g in finetune.BatchLoader(Set(), [], workers=1)] == []


def test_collate_stacks_and_refuses_mixed_sizes():
    def sample(h, w, tag):
        return {"imgs": torch.full((3, 3, h, w), float(tag)), "name": f"s{tag}",
                "proj_matrix": {f"stage{s}": np.full((3, 2, 4, 4), tag + s, np.float32) for s in (1, 2, 3)},
                "depth_values": np.arange(4, dtype=np.float32) + tag, "depth_interval": 2.5 + tag,
                "depth": {f"stage{s}": torch.full((h >> (3 - s), w >> (3 - s)), float(tag)) for s in (1, 2, 3)},
                "mask": {f"stage{s}": torch.ones(h >> (3 - s), w >> (3 - s)) for s in (1, 2, 3)}}

    one = finetune.collate(sample(8, 12, 0), "cpu")
    assert one["imgs"].shape == (1, 3, 3, 8, 12) and one["depth_values"].shape == (1, 4)
    assert one["proj_matrix"]["stage2"].shape == (1, 3, 2, 4, 4) and one["depth_interval"] == 2.5
    same = finetune.collate([sample(8, 12, 0)], "cpu")
    assert all(torch.equal(one[k], same[k]) for k in ("imgs", "depth_values"))
    two = finetune.collate([sample(8, 12, 0), sample(8, 12, 1)], "cpu")
    assert two["imgs"].shape == (2, 3, 3, 8, 12) and two["depth"]["stage1"].shape == (2, 2, 3)
    assert two["depth_values"][1, 0] == 1 and two["proj_matrix"]["stage3"][1, 0, 0, 0, 0] == 4
    assert float(two["imgs"][1].min()) == 1.0 and two["depth_interval"].tolist() == [2.5, 3.5]
    with pytest.raises(ValueError, match="one image size"):
        finetune.collate([sample(8, 12, 0), sample(8, 16, 1)], "cpu")
