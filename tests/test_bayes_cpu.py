"""--loss bayes on the command line and in the plumbing, without a GPU: what the parser refuses, and that the default
(--loss mse) hands the loaders' launch and the stepper exactly the arguments it handed them before the flag existed."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = ["--crop-size", "64x96", "--gt-from-heads", "--loss", "bayes"]


@pytest.fixture(scope="module")
def parser():
    sys.path.insert(0, ROOT)
    try:
        import train
    finally:
        sys.path.remove(ROOT)
    return train.build_parser()


def test_parser_accepts(parser):
    a = parser.parse_args([])
    assert (a.loss, a.bayes_sigma, a.bayes_bg) == ("mse", 8.0, 0.15)
    a = parser.parse_args(OK + ["--bayes-sigma", "4", "--bayes-bg", "0", "--graph", "auto", "--dtype", "fp16"])
    assert (a.loss, a.bayes_sigma, a.bayes_bg) == ("bayes", 4.0, 0.0)


@pytest.mark.parametrize("argv", [
    ["--crop-size", "64x96", "--loss", "bayes"], OK + ["--impl", "torch"], OK + ["--dtype", "fp32"],
    OK + ["--gpu-preprocess", "0"], OK + ["--roi-masks"], OK + ["--graph", "1"], OK + ["--bayes-sigma", "0"],
    OK + ["--bayes-sigma", "nan"], OK + ["--bayes-bg", "-0.1"], OK + ["--bayes-bg", "1.5"], ["--loss", "l1"]])
def test_parser_refuses(parser, argv):
    with pytest.raises(SystemExit):
        parser.parse_args(argv)


def test_mse_keeps_todays_arguments(monkeypatch):
    from can_distributed_pytorch_amd.engine import native, trainer
    from can_distributed_pytorch_amd.ops import _ext, preprocess
    seen = {}
    monkeypatch.setattr(native, "NativeStepper", lambda *a, **kw: seen.update(stepper=kw))
    trainer.build_trainer(impl="hip", dtype="bf16", device="cpu")
    assert not {"loss", "bayes_sigma", "bayes_bg"} & set(seen["stepper"])
    trainer.build_trainer(impl="hip", dtype="bf16", device="cpu", loss="bayes", bayes_sigma=4.0)
    assert seen["stepper"]["loss"] == "bayes" and seen["stepper"]["bayes_sigma"] == 4.0
    for kw in (dict(impl="torch"), dict(impl="hip", dtype="fp32")):
        with pytest.raises(ValueError):
            trainer.build_trainer(device="cpu", loss="bayes", **kw)
    monkeypatch.setattr(_ext, "require", lambda: None)
    monkeypatch.setattr(preprocess, "_launch", lambda *a, **kw: seen.update(launch=kw))
    packed = preprocess.PackedCollate()([(torch.zeros(16, 24, 3, dtype=torch.uint8), torch.zeros(1, 2, 3), False)])
    preprocess.preprocess_packed(packed, "cpu")
    assert seen["launch"] == {"roi": False}
    preprocess.preprocess_packed(packed, "cpu", points=True)
    assert seen["launch"] == {"roi": False, "points": True}
