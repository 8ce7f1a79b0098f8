"""Optimizer choice (SGD + weight decay, Adam, AdamW) on the CPU side: the arena rehearsal stepper against
torch.optim, the skip on a non-finite loss, the train-state round trip, the command line and the custom operator's
registration."""
import copy
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = [("adam", torch.optim.Adam, {}), ("adamw", torch.optim.AdamW, {}),
         ("sgd", torch.optim.SGD, {"momentum": 0.95})]


def _model(seed=0):
    from can_distributed_pytorch_amd.models import CANNet
    torch.manual_seed(seed)
    return CANNet(backend="torch")


@pytest.mark.parametrize("name,cls,kw", CASES, ids=[c[0] for c in CASES])
def test_arena_stepper_matches_torch_optim(name, cls, kw):
    """Three ArenaStepper steps == torch.optim on a deep copy fed the stepper's own arena gradients (an independent
    backward would not do: Adam normalises the gradient magnitude away, so two near-zero gradients of opposite
    rounding differ by a full lr)."""
    from can_distributed_pytorch_amd.engine.trainer import ArenaStepper
    lr = 1e-4
    m = _model()
    ref = copy.deepcopy(m)
    st = ArenaStepper("cpu", lr=lr, model=m, optimizer=name, weight_decay=5e-4)
    opt = cls(ref.parameters(), lr=lr, weight_decay=5e-4, **kw)
    img, gt = torch.randn(1, 3, 64, 64), torch.rand(1, 1, 8, 8)
    for _ in range(3):
        st.step(img, gt)
        for p, q in zip(m.parameters(), ref.parameters()):
            q.grad = p.grad.detach().clone()
        opt.step()
    moved = 0.0
    for (n, p), q, p0 in zip(m.named_parameters(), ref.parameters(), _model().parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6 * lr), (n, float((p - q).abs().max()))
        moved = max(moved, float((p.detach() - p0.detach()).abs().max()))
    assert moved > 0
    if name != "sgd":
        assert st.opt_steps == 3


@pytest.mark.parametrize("name", ["adam", "adamw", "sgd"])
def test_arena_stepper_skips_nonfinite_loss(name):
    from can_distributed_pytorch_amd.engine.trainer import ArenaStepper
    m = _model(1)
    st = ArenaStepper("cpu", lr=1e-4, model=m, optimizer=name, weight_decay=5e-4)
    img, gt = torch.randn(1, 3, 64, 64), torch.rand(1, 1, 8, 8)
    st.step(img, gt)
    w, m1 = st.arena.data.clone(), st.mom.clone()
    m2 = None if st.mom2 is None else st.mom2.clone()
    t = st.opt_steps
    bad = gt.clone()
    bad[0, 0, 0, 0] = float("inf")
    loss = st.step(img, bad)
    assert not bool(torch.isfinite(loss).all())
    assert torch.equal(st.arena.data, w) and torch.equal(st.mom, m1) and st.opt_steps == t
    if m2 is not None:
        assert torch.equal(st.mom2, m2)


def test_train_state_round_trip_and_mismatch(tmp_path):
    from can_distributed_pytorch_amd.utils.checkpoint import save_train_state, load_train_state
    m = _model(2)
    n = 1000
    mom, mom2 = torch.randn(n), torch.rand(n)
    path = str(tmp_path / "last_state.pth")
    save_train_state(path, m, mom, 3, 1.5, stepper_state={"lr": 1e-4, "steps": 7, "optimizer": "adam", "opt_steps": 5},
                     momentum2=mom2, optimizer_name="adam")
    a, b = torch.zeros(n), torch.zeros(n)
    rs = load_train_state(path, _model(3), a, momentum2=b, optimizer_name="adam", restore_rng=False)
    assert torch.equal(a, mom) and torch.equal(b, mom2)
    assert rs["epoch"] == 3 and rs["stepper"]["opt_steps"] == 5 and rs["stepper"]["optimizer"] == "adam"
    with pytest.raises(ValueError, match="adam"):
        load_train_state(path, _model(3), a, optimizer_name="sgd", restore_rng=False)
    with pytest.raises(ValueError, match="adam"):
        load_train_state(path, _model(3), a, momentum2=b, optimizer_name="adamw", restore_rng=False)
    # a state in the earlier format (no second moment, no optimizer name) is an SGD state
    st = torch.load(path, weights_only=True)
    del st["momentum2"], st["optimizer_name"]
    st["stepper"] = {"lr": 1e-4, "steps": 7}
    old = str(tmp_path / "old_state.pth")
    torch.save(st, old)
    c = torch.zeros(n)
    rs = load_train_state(old, _model(3), c, optimizer_name="sgd", restore_rng=False)
    assert torch.equal(c, mom) and rs["stepper"]["steps"] == 7
    load_train_state(old, _model(3), c, restore_rng=False)          # the earlier call form still works
    with pytest.raises(ValueError, match="sgd"):
        load_train_state(old, _model(3), c, momentum2=b, optimizer_name="adam", restore_rng=False)


def test_parser_accepts_optimizer_flags_and_keeps_defaults():
    import train
    p = train.build_parser()
    d = p.parse_args([])
    assert (d.optimizer, d.momentum, d.weight_decay, d.beta1, d.beta2, d.eps, d.lr) == \
        ("sgd", 0.95, 0.0, 0.9, 0.999, 1e-8, 1e-7)
    a = p.parse_args(["--optimizer", "adamw", "--momentum", "0.9", "--weight-decay", "1e-2", "--beta1", "0.8",
                      "--beta2", "0.99", "--eps", "1e-6"])
    assert (a.optimizer, a.momentum, a.weight_decay, a.beta1, a.beta2, a.eps) == ("adamw", 0.9, 1e-2, 0.8, 0.99, 1e-6)
    with pytest.raises(SystemExit):
        p.parse_args(["--optimizer", "lion"])


def test_torch_stepper_builds_the_chosen_optimizer():
    from can_distributed_pytorch_amd.engine.trainer import build_trainer
    for name, cls in (("sgd", torch.optim.SGD), ("adam", torch.optim.Adam), ("adamw", torch.optim.AdamW)):
        st = build_trainer(impl="torch", dtype="fp32", device="cpu", lr=1e-5, model=_model(), optimizer=name,
                           weight_decay=1e-2, betas=(0.8, 0.99), eps=1e-6, momentum=0.9)
        g = st.opt.param_groups[0]
        assert type(st.opt) is cls and g["weight_decay"] == 1e-2 and g["lr"] == 1e-5
        if name == "sgd":
            assert g["momentum"] == 0.9
        else:
            assert tuple(g["betas"]) == (0.8, 0.99) and g["eps"] == 1e-6
    d = build_trainer(impl="torch", dtype="fp32", device="cpu", model=_model()).opt
    assert type(d) is torch.optim.SGD and d.param_groups[0]["momentum"] == 0.95 and \
        d.param_groups[0]["weight_decay"] == 0


def test_adam_op_registered_with_fake_impl():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import can_distributed_pytorch_amd.ops.library  # noqa: F401
    op = torch.ops.cannet.adam_
    schema = str(op.default._schema)
    for arg in ("param", "exp_avg", "exp_avg_sq", "grad", "step", "lr", "beta1", "beta2", "eps", "weight_decay",
                "decoupled", "grad_scale"):
        assert arg in schema, schema
    with FakeTensorMode():
        p, m, v, g = (torch.empty(1000) for _ in range(4))
        assert op(p, m, v, g, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, False, 1.0) is None
