"""GPU: the device measurement learner (csrc/qcart_mlearner.hip through MeasurementLearner) against the
torch-on-CPU restatement tests/mlearner_ref.py on identical parameters, rows and noise.

Geometry: L = 500, m = 50 (K = 10, row_len 563): T = 98 / 22 / 4 with remainders 2 / 3 / 1, so every convolution
has uncovered trailing inputs, no T is a multiple of 32 (column tiles cross env boundaries) and the stride-4
phases have 3 / 2 / 2 / 2 (KS = 9) and 3 / 3 / 3 / 2 (KS = 11) taps. Non-zero conv and fc biases; a few rows with
a partly zero history.

Tolerances. The kernels compute in fp32 with exact-f32 MFMA accumulation, the restatement in fp64:
  * per-sample losses: <= 2e-5 max|ul| + 1e-5 (test_gpu_learner.py), on rows whose top-two gap of Q_online(next)
    exceeds twice that tolerance;
  * gradients, per tensor: <= tol max|g_ref|, tol = max(2e-5, 8 r32), r32 that tensor's max-norm distance
    between the restatement in fp32 and in fp64 on the CPU (R32 / R32_DRIVER below; never from the device);
  * LaProp: <= 1e-5 lr + 2^-23 |p| per step.
"""
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import learner_ref as R  # noqa: E402
from tests import mlearner_ref as M  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd._lib import QCartError  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.actor import (MeasurementActor,  # noqa: E402
                                                                          random_direct_dqn)
from deepreinforcementlearningcontrolofquantumcartpoles_amd.learner import MeasurementLearner  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.replay import PrioritizedReplay  # noqa: E402

L, MS, B = 500, 50, 128
LR = 4e-4

# python -m tests.mlearner_ref 500 50 128   (max|g32 - g64| / max|g64| of the restatement, CPU)
R32 = {
    "conv1.weight": 4.7e-07, "conv1.bias": 7.6e-07, "conv2.weight": 6.9e-07, "conv2.bias": 5.2e-07,
    "conv3.weight": 6.1e-07, "conv3.bias": 3.5e-07, "fc1.weight": 3.9e-07, "fc1.bias": 2.5e-07,
    "fc21.u_w": 5.3e-07, "fc21.sigma_w": 5.1e-07, "fc21.u_b": 1.5e-07, "fc21.sigma_b": 3.6e-07,
    "fc31.u_w": 3.3e-07, "fc31.sigma_w": 2.3e-07, "fc31.u_b": 1.8e-07, "fc31.sigma_b": 3.2e-07,
    "fc22.weight": 5.1e-07, "fc22.bias": 1.4e-07, "fc22.weight_norm": 8.3e-07,
    "fc32.weight": 3.1e-07, "fc32.bias": 4.0e-08, "fc32.weight_norm": 1.0e-06,
}
# python -m tests.mlearner_ref 5760 80 128
R32_DRIVER = {
    "conv1.weight": 1.5e-04, "conv1.bias": 2.2e-04, "conv2.weight": 9.8e-07, "conv2.bias": 2.5e-06,
    "conv3.weight": 8.7e-07, "conv3.bias": 1.3e-06, "fc1.weight": 4.6e-07, "fc1.bias": 1.6e-07,
    "fc21.u_w": 3.2e-07, "fc21.sigma_w": 5.5e-07, "fc21.u_b": 1.4e-07, "fc21.sigma_b": 2.3e-07,
    "fc31.u_w": 3.1e-07, "fc31.sigma_w": 3.4e-07, "fc31.u_b": 7.3e-08, "fc31.sigma_b": 2.0e-07,
    "fc22.weight": 3.1e-07, "fc22.bias": 1.1e-07, "fc22.weight_norm": 3.7e-07,
    "fc32.weight": 1.1e-07, "fc32.bias": 2.3e-08, "fc32.weight_norm": 9.7e-08,
}


def cuda(x):
    return torch.as_tensor(np.asarray(x)).cuda()


def host(d):
    return {k: v.detach().cpu() for k, v in d.items()}


def digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def case():
    """Parameters, one batch, and the fp64 restatement of its first update (computed once, never modified)."""
    p = M.random_params(L, seed=5)
    tr, w, nz = M.make_batch(B, 3, L, MS)
    ul, loss, g, qn = M.loss_and_grads(p, p, tr, w, nz, L, MS)
    return {"p": p, "tr": tr, "w": w, "nz": nz, "ul": ul, "loss": loss, "g": g, "qn": qn}


def make(p, **kw):
    kw.setdefault("lr", LR)
    return MeasurementLearner(p, L, MS, batch_size=kw.pop("batch_size", B), **kw)


def top_two_gap(q):
    s = np.sort(q, axis=1)
    return s[:, -1] - s[:, -2]


def check_params(dev, ref, lr, steps, what=""):
    for k, r in ref.items():
        r = r.double().numpy()
        err = np.abs(dev[k].double().numpy() - r)
        tol = steps * (1e-5 * lr + 2.0 ** -23 * np.abs(r))
        assert (err <= tol).all(), (what, k, float((err - tol).max()), float(err.max()))


# ---- state assembly ------------------------------------------------------------------------------------------
def test_states_are_bitwise_the_restatement(case):
    ln = make(case["p"])
    nxt, prv = ln.states(cuda(case["tr"]))
    rn, rp = M.assemble(torch.as_tensor(case["tr"]), L, MS)
    assert torch.equal(nxt.cpu(), rn) and torch.equal(prv.cpu(), rp)


# ---- loss ----------------------------------------------------------------------------------------------------
def test_loss_matches_restatement(case):
    ln = make(case["p"], lr=0.0)
    ul = ln.update(cuda(case["tr"]), cuda(case["w"]), cuda(case["nz"])).cpu().double().numpy()
    tol = 2e-5 * np.abs(case["ul"]).max() + 1e-5
    ok = top_two_gap(case["qn"]) > 2 * tol
    assert ok.sum() > B // 2
    err = np.abs(ul - case["ul"])
    print("max ul err", err[ok].max(), "tol", tol)
    assert (err[ok] <= tol).all()
    if ok.all():
        assert abs(float(ln.last_loss.cpu()) - case["loss"]) <= tol
    assert ln.stats()["launches_per_update"] == 30   # 28 launches + the 2 target copies of the first update


# ---- gradients -----------------------------------------------------------------------------------------------
def grad_check(g_dev, g_ref, r32):
    assert len(g_ref) == 22 and set(g_dev) == set(g_ref)
    bad = {}
    for k, r in g_ref.items():
        tol = max(2e-5, 8 * r32[k])
        err = float(np.abs(g_dev[k].double().numpy().reshape(r.shape) - r).max() / np.abs(r).max())
        print(f"{k:18s} err {err:.2e} tol {tol:.1e}")
        if not err <= tol:
            bad[k] = (err, tol)
    assert not bad, bad


def test_gradients_match_autograd(case):
    """lr = 0: the update leaves the parameters where they are and grads() holds the gradients of the raw
    parameters (the weight-norm chain rule applied)."""
    assert (top_two_gap(case["qn"]) > 1e-4).all(), "a borderline argmax would change a target"
    ln = make(case["p"], lr=0.0)
    ln.update(cuda(case["tr"]), cuda(case["w"]), cuda(case["nz"]))
    grad_check(host(ln.grads()), case["g"], R32)


def test_uncovered_inputs_and_batch_256(case):
    """B = 256 (two rows per noise chunk more, another split-K shape): gradients against autograd again."""
    p = case["p"]
    tr, w, nz = M.make_batch(256, 3, L, MS)
    _, _, g, qn = M.loss_and_grads(p, p, tr, w, nz, L, MS)
    assert (top_two_gap(qn) > 1e-4).all()
    ln = make(p, lr=0.0, batch_size=256)
    ln.update(cuda(tr), cuda(w), cuda(nz))
    grad_check(host(ln.grads()), g, R32)


def test_driver_geometry():
    """L = 5760, m = 80 (MeasurementRecord's for the IHO defaults), B = 128: T = 1150 / 285 / 70. It exists for
    offsets, grid sizes and the split-K at scale. Its bounds are loose by the tolerance rule: fp32 rounding alone
    reaches 1.5e-4 for conv1.weight and 2.2e-4 for conv1.bias in the CPU fp32 run (R32_DRIVER), so it cannot stand in for the
    small geometry, where one missed position is 1e-2."""
    Ld, md = 5760, 80
    p = M.random_params(Ld, seed=5)       # r32_table's inputs
    tr, w, nz = M.make_batch(128, 3, Ld, md)
    _, _, g, qn = M.loss_and_grads(p, p, tr, w, nz, Ld, md)
    assert (top_two_gap(qn) > 1e-4).all()
    ln = MeasurementLearner(p, Ld, md, batch_size=128, lr=0.0)
    ln.update(cuda(tr), cuda(w), cuda(nz))
    grad_check(host(ln.grads()), g, R32_DRIVER)


# ---- optimizer and schedule ----------------------------------------------------------------------------------
def test_apply_is_laprop(case):
    p = case["p"]
    ln = make(p)
    ref = R.LaProp(p, lr=LR)
    gen = torch.Generator().manual_seed(5)
    for step in range(1, 13):        # crosses the centred switch (step 11)
        grads = {k: torch.randn(v.shape, generator=gen) * 10.0 ** float(torch.randint(-4, 1, (1,), generator=gen))
                 for k, v in p.items()}
        ln.apply({k: v.cuda() for k, v in grads.items()})
        ref.step(grads)
        dev = host(ln.state_dict())
        check_params(dev, ref.p, LR, 1, f"step {step}")
        # the bound is one step's: the next step starts from the device's parameters (the fp64 e, v, mu carry on)
        ref.p = {k: v.double() for k, v in dev.items()}
    st = ln.stats()
    assert st["step"] == 12 and abs(st["l1"] - ref.l1) < 1e-15 and abs(st["l2"] - ref.l2) < 1e-15


def test_twelve_updates_and_target_schedule(case):
    """12 updates, backup_period 5: after an update whose position in the period is 0 the target is, bitwise,
    the online net that update started from; every update is LaProp on its own gradients (one step's tolerance,
    the next step starts from the device's parameters), and those gradients are autograd's for the device's
    online and target parameters (the gradient rule above), so the target fragments are the target's."""
    p = case["p"]
    ln = make(p, backup_period=5)
    tr, w, nz = cuda(case["tr"]), cuda(case["w"]), cuda(case["nz"])
    opt = R.LaProp(p, lr=LR)
    target, counter = None, 0
    for n in range(12):
        before = host(ln.state_dict())
        refresh = counter == 0
        counter = (counter + 1) % 5
        ul = ln.update(tr, w, nz).cpu().double().numpy()
        tgt = host(ln.state_dict(target=True))
        if refresh:
            assert all(torch.equal(tgt[k], before[k]) for k in tgt), n
            target = before
        else:
            assert all(torch.equal(tgt[k], target[k]) for k in tgt), n
        g_dev = host(ln.grads())
        ul_ref, _, g_ref, qn = M.loss_and_grads(before, target, case["tr"], case["w"], case["nz"], L, MS)
        tol = 2e-5 * np.abs(ul_ref).max() + 1e-5
        if (top_two_gap(qn) > 2 * tol).all():   # else a borderline argmax changes a target
            assert (np.abs(ul - ul_ref) <= tol).all(), n
            grad_check(g_dev, g_ref, R32)
        opt.p = R.to_params(before, torch.float64)
        opt.step({k: v.double() for k, v in g_dev.items()})
        check_params(host(ln.state_dict()), opt.p, LR, 1, f"update {n}")
    s = ln.stats()
    assert s["updates"] == 12 and s["step"] == 12 and s["backup_counter"] == 12 % 5 and s["nonfinite"] == 0
    assert s["launches_per_update"] == 28


# ---- determinism ---------------------------------------------------------------------------------------------
def test_same_inputs_give_bit_identical_parameters(case):
    out = []
    for _ in range(2):
        ln = make(case["p"], seed=7)
        tr, w = cuda(case["tr"]), cuda(case["w"])
        for n in range(8):
            ln.update(tr, w, counter=n)
        out.append(digest(ln.state_dict()))
    assert out[0] == out[1]
    a, b = make(case["p"], seed=7), make(case["p"], seed=7)
    ua = a.update(cuda(case["tr"]), cuda(case["w"]), counter=0)
    ub = b.update(cuda(case["tr"]), cuda(case["w"]), counter=1)
    assert not torch.equal(ua, ub)


def test_fixed_batch_loss_falls(case):
    ln = make(case["p"], backup_period=50)
    tr, w, nz = cuda(case["tr"]), cuda(case["w"]), cuda(case["nz"])
    losses = []
    for n in range(200):
        ln.update(tr, w, nz)
        if n % 10 == 0 or n == 199:
            losses.append(float(ln.last_loss.cpu()))
    print(losses)
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0]
    assert ln.stats()["nonfinite"] == 0


# ---- wiring --------------------------------------------------------------------------------------------------
def test_record_replay_step_push(case):
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import config as cfg
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.core import Stepper
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.measurements import MeasurementRecord
    nb = 64
    ph = cfg.DEFAULTS[cfg.IHO].with_(n_max=63, time_steps=1800, n_con=18)   # control interval 100 = 2 MS
    st = Stepper(ph, nb, 0, seed=3)
    psi = st.new_state()
    st.reset(psi, 1, arg0=4)
    rec = MeasurementRecord(st, read_length=L, coarse_grain=2)
    assert rec.m == MS and rec.row_len == M.row_len(L, MS)
    mem = PrioritizedReplay(1024, rec.row_len, seed=2)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.zeros((nb, rec.row_len), dtype=torch.float32, device="cuda")
    reward = torch.ones(nb, dtype=torch.float32, device="cuda")
    for it in range(3):
        acts = torch.randint(0, 21, (nb,), generator=gen, device="cuda", dtype=torch.int32)
        o = st.step(psi, acts, ph.control_interval, want_q=True)
        mode = torch.full((nb,), 2 if it == 0 else 1, dtype=torch.uint8, device="cuda")
        rec.record(o["q"], actions=acts, mode=mode, reward=reward, rows=rows)
        mem.store(rows)
    ln = make(case["p"])
    assert ln.step(mem) is not None
    sd = ln.state_dict()
    a = MeasurementActor({k: v.cpu() for k, v in case["p"].items()}, read_length=L, max_batch=nb, seed=1)
    ln.push(a)
    b = MeasurementActor(sd, read_length=L, max_batch=nb, seed=1)
    aa, ea = a.act(rec.hist, counter=3, want_q=True)
    ab, eb = b.act(rec.hist, counter=3, want_q=True)
    assert torch.equal(aa, ab) and torch.equal(ea["q"], eb["q"])
    other = MeasurementActor(M.random_params(600, seed=1), read_length=600, max_batch=nb)
    with pytest.raises(ValueError):
        ln.push(other)


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals(case):
    p = case["p"]
    for bs in (100, 1152):
        with pytest.raises(ValueError):
            make(p, batch_size=bs)
    with pytest.raises(ValueError):
        MeasurementLearner(p, L, 70, batch_size=B)
    wn = dict(p)
    wn["conv2.weight_norm"] = p["conv2.weight"].norm()
    with pytest.raises(QCartError, match="conv2"):
        make(wn)
    bad = dict(p)
    bad["fc1.weight"] = p["fc1.weight"][:, :-1]
    with pytest.raises(ValueError):
        make(bad)
    with pytest.raises(ValueError):
        make(random_direct_dqn(data_length=5, seed=1))
    with pytest.raises(RuntimeError):
        make(p, device="cpu")
    ln = make(p)
    with pytest.raises(ValueError):
        ln.update(cuda(case["tr"])[:, :-1], cuda(case["w"]))
    with pytest.raises(ValueError):
        ln.update(cuda(case["tr"]), cuda(case["w"]), torch.zeros(32, 10))
    tr = case["tr"].copy()
    tr[5, -2] = 40.0
    ln.update(cuda(tr), cuda(case["w"]), cuda(case["nz"]))
    with pytest.raises(QCartError):
        ln.stats()
    ln.stats()   # reported once
