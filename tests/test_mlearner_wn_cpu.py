"""CPU: the restatement of the weight-normalised measurement learner (tests/mlearner_wn_ref.py) checked on its own:
the convolutions' weight and weight_norm gradients against central finite differences in fp64 on a tiny geometry;
on the GPU tests' own inputs, that the two mistakes a device path can make (acting on the raw W, or on W g without
dividing by ||W||_F) move the action values, the per-sample losses and the convolutions' gradients by more than
100 of the GPU tests' tolerances, so those tests tell them apart; and the library's argument check of
conv_weight_norm, which holds without a GPU."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import mlearner_ref as M  # noqa: E402
from tests import mlearner_wn_ref as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepreinforcementlearningcontrolofquantumcartpoles_amd", "libqcart.so")

LT, MT, BT = 300, 30, 32   # T = 58 / 12 / 1
L, MS, B, SEED, PSEED = 500, 50, 128, 2, 5   # tests/test_gpu_mlearner_wn.py's small geometry and seeds
CONV_KEYS = [f"{n}.{k}" for n in W.CONV_NAMES for k in ("weight", "weight_norm")]


def test_random_params_are_trained_like():
    p = W.random_params(L, seed=PSEED)
    assert len(p) == 25
    scales = [float(p[f"{n}.weight_norm"] / p[f"{n}.weight"].norm()) for n in W.CONV_NAMES]
    assert all(0.7 <= s <= 1.4 and abs(s - 1) > 0.02 for s in scales), scales
    assert min(abs(a - b) for i, a in enumerate(scales) for b in scales[:i]) > 0.02, scales
    assert all(float(p[f"{n}.bias"].abs().min()) > 0 for n in W.CONV_NAMES)
    plain = W.random_params(L, seed=PSEED, conv_weight_norm=False)
    ref = M.random_params(L, seed=PSEED)
    assert set(plain) == set(ref) and all(torch.equal(plain[k], ref[k]) for k in ref)


def test_plain_parameters_pass_through_unchanged():
    p = M.random_params(LT, seed=2)
    tr, w, nz = M.make_batch(BT, 4, LT, MT)
    a = M.loss_and_grads(p, p, tr, w, nz, LT, MT)
    b = W.loss_and_grads(p, p, tr, w, nz, LT, MT, target="alive")
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])


@pytest.mark.parametrize("target", ["reward", "alive"])
def test_conv_gradients_match_central_differences(target):
    p = W.random_params(LT, seed=2)
    tr, w, nz = W.make_batch(BT, 4, LT, MT, target)
    _, _, g, _ = W.loss_and_grads(p, p, tr, w, nz, LT, MT, target=target)
    assert len(g) == 25
    p64 = {k: v.double() for k, v in p.items()}
    t = lambda a: torch.as_tensor(np.asarray(a)).double()   # noqa: E731
    rng = np.random.default_rng(0)
    h = 1e-6
    for k in CONV_KEYS + ["conv1.bias", "fc1.weight", "fc22.weight_norm"]:
        flat = p64[k].reshape(-1)
        for i in rng.choice(flat.numel(), size=min(4, flat.numel()), replace=False):
            vals = []
            for sgn in (1.0, -1.0):
                q = {kk: vv.clone() for kk, vv in p64.items()}
                q[k].reshape(-1)[i] += sgn * h
                vals.append(float(W.td_loss(q, p64, t(tr), t(w), t(nz), LT, MT, target=target)[0]))
            fd = (vals[0] - vals[1]) / (2 * h)
            ref = float(g[k].reshape(-1)[i])
            assert abs(fd - ref) <= 1e-6 * max(1.0, abs(ref)) + 1e-7 * np.abs(g[k]).max(), (k, int(i), fd, ref)


def test_weight_gradient_is_orthogonal_to_the_weight():
    """The effective weight depends on W only through its direction: <dL/dW, W> = 0 for each convolution."""
    p = W.random_params(LT, seed=2)
    tr, w, nz = W.make_batch(BT, 4, LT, MT, "reward")
    _, _, g, _ = W.loss_and_grads(p, p, tr, w, nz, LT, MT, target="reward")
    for n in W.CONV_NAMES:
        wt = p[f"{n}.weight"].double().numpy()
        dot = float((g[f"{n}.weight"] * wt).sum())
        assert abs(dot) <= 1e-12 * float(np.abs(g[f"{n}.weight"]).max() * np.abs(wt).sum()), (n, dot)


@pytest.fixture(scope="module")
def gpu_case():
    """The GPU tests' inputs, the restatement on them, and r32 of the convolutions' gradients."""
    p = W.random_params(L, seed=PSEED)
    tr, w, nz = W.make_batch(B, SEED, L, MS, "reward")
    ul, _, g, _ = W.loss_and_grads(p, p, tr, w, nz, L, MS, target="reward")
    obs = M.assemble(torch.as_tensor(tr[:64]), L, MS)[0].numpy()
    return {"p": p, "tr": tr, "w": w, "nz": nz, "ul": ul, "g": g, "obs": obs, "q": W.actor_q(p, obs),
            "r32": W.r32_table(L, MS, B, seed=SEED, pseed=PSEED, target="reward")}


@pytest.mark.parametrize("mistake", ["raw", "no_norm"])
def test_mistakes_are_visible_at_the_gpu_tolerances(gpu_case, mistake):
    c = gpu_case
    q_bad = W.actor_q(c["p"], c["obs"], mistake=mistake)
    q_tol = 5e-5 * np.abs(c["q"]).max() + 1e-5                      # tests/test_gpu_mactor.py
    assert np.abs(q_bad - c["q"]).max() > 100 * q_tol
    ul_bad, _, g_bad, _ = W.loss_and_grads(c["p"], c["p"], c["tr"], c["w"], c["nz"], L, MS, target="reward",
                                           mistake=mistake) if mistake != "raw" else _raw(c)
    ul_tol = 2e-5 * np.abs(c["ul"]).max() + 1e-5
    assert np.abs(ul_bad - c["ul"]).max() > 100 * ul_tol
    for k in CONV_KEYS:
        tol = max(2e-5, 8 * c["r32"][k])
        err = np.abs(g_bad[k] - c["g"][k]).max() / np.abs(c["g"][k]).max()
        assert err > 100 * tol, (k, err, tol)


def _raw(c):
    """The raw-W mistake: the loss does not depend on weight_norm, whose gradient is then zero."""
    p = {k: v for k, v in c["p"].items() if not (k.startswith("conv") and k.endswith("weight_norm"))}
    ul, loss, g, qn = W.loss_and_grads(p, p, c["tr"], c["w"], c["nz"], L, MS, target="reward")
    for n in W.CONV_NAMES:
        g[f"{n}.weight_norm"] = np.zeros(())
    return ul, loss, g, qn


@pytest.mark.skipif(not os.path.exists(LIB), reason="libqcart.so not built")
@pytest.mark.parametrize("flag", [2, -1])
def test_create_refuses_a_bad_conv_weight_norm(flag):
    """The argument checks come before the device is looked at: they hold without a GPU."""
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
    p = _lib.QcMlearnerParams()
    p.read_length, p.read_step_length, p.n_actions, p.batch_size = 500, 50, 21, 128
    p.backup_period, p.target_mode, p.gamma, p.lr = 300, 2, 0.998, 4e-4
    p.conv_weight_norm = flag
    h = ctypes.c_void_p()
    assert _lib.lib().qc_mlearner_create(ctypes.byref(p), 0, ctypes.byref(h)) == -1 and not h.value
    assert "conv_weight_norm" in _lib.lib().qc_mlearner_last_error(None).decode()


def test_random_dqn_measurement_keyword():
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.actor import random_dqn_measurement
    a = random_dqn_measurement(read_length=500, seed=3)
    b = random_dqn_measurement(read_length=500, seed=3, conv_weight_norm=True)
    assert set(b) - set(a) == {f"{n}.weight_norm" for n in W.CONV_NAMES}
    assert all(torch.equal(a[k], b[k]) for k in a)
    for n in W.CONV_NAMES:
        assert torch.equal(b[f"{n}.weight_norm"], b[f"{n}.weight"].norm())
