"""--loss dmcount on the command line and in the plumbing, without a GPU, and the reference's own Sinkhorn: after the
last update of u the transport plan has the prediction's marginal."""
import os
import sys

import numpy as np
import pytest

from dmcount_reference import reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = ["--crop-size", "64x96", "--gt-from-heads", "--loss", "dmcount"]


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
    assert (a.loss, a.ot_reg, a.ot_iters, a.ot_weight, a.tv_weight) == ("mse", 10.0, 100, 0.1, 0.01)
    a = parser.parse_args(OK + ["--ot-reg", "1", "--ot-iters", "7", "--ot-weight", "0", "--tv-weight", "2",
                                "--graph", "auto", "--dtype", "fp16"])
    assert (a.loss, a.ot_reg, a.ot_iters, a.ot_weight, a.tv_weight) == ("dmcount", 1.0, 7, 0.0, 2.0)


@pytest.mark.parametrize("argv", [
    ["--crop-size", "64x96", "--loss", "dmcount"], OK + ["--impl", "torch"], OK + ["--dtype", "fp32"],
    OK + ["--gpu-preprocess", "0"], OK + ["--roi-masks"], OK + ["--graph", "1"], OK + ["--ot-reg", "0.5"],
    OK + ["--ot-reg", "101"], OK + ["--ot-reg", "nan"], OK + ["--ot-iters", "0"], OK + ["--ot-iters", "1001"],
    OK + ["--ot-weight", "-1"], OK + ["--tv-weight", "inf"]])
def test_parser_refuses(parser, argv):
    with pytest.raises(SystemExit):
        parser.parse_args(argv)


def test_parameters_reach_the_stepper(monkeypatch):
    from can_distributed_pytorch_amd.engine import native, trainer
    seen = {}
    monkeypatch.setattr(native, "NativeStepper", lambda *a, **kw: seen.update(stepper=kw))
    trainer.build_trainer(impl="hip", dtype="bf16", device="cpu", loss="dmcount", ot_reg=2.0, ot_iters=5)
    kw = seen["stepper"]
    assert (kw["loss"], kw["ot_reg"], kw["ot_iters"], kw["ot_weight"], kw["tv_weight"]) == ("dmcount", 2.0, 5, 0.1, 0.01)
    assert not {"bayes_sigma", "bayes_bg"} & set(kw)
    trainer.build_trainer(impl="hip", dtype="bf16", device="cpu", loss="bayes")
    assert not {"ot_reg", "ot_iters", "ot_weight", "tv_weight"} & set(seen["stepper"])
    for bad in (dict(impl="torch"), dict(impl="hip", dtype="fp32")):
        with pytest.raises(ValueError):
            trainer.build_trainer(device="cpu", loss="dmcount", **bad)


@pytest.mark.parametrize("reg,iters", [(10.0, 100), (1.0, 1)])
def test_reference_marginal(reg, iters):
    rng = np.random.default_rng(0)
    et = rng.uniform(-1.0, 1.0, (5, 7))
    pts = np.stack([rng.uniform(0, 56, 9), rng.uniform(0, 40, 9)], 1)
    r = reference(et, pts, reg, iters)
    assert np.allclose((r["K"] * r["v"][:, None]).sum(0) * r["u"], r["a"], rtol=1e-12, atol=0)
