"""CPU: the checker of the DQN variants (tests/dqn_variants_ref.py: fc2 of width 512, the three TD targets)
against explicit per-row restatements, hand-computed targets and finite differences; random_direct_dqn's wide
net; and the qc_dqn_params mirror against the header."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from tests import dqn_variants_ref as V  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.actor import random_direct_dqn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p64(**kw):
    return V.to_params(random_direct_dqn(seed=11, **kw), torch.float64)


def test_random_wide_net_shapes():
    p = random_direct_dqn(data_length=7, n_actions=21, hidden2=512, seed=3)
    want = {"fc1.weight": (512, 7), "fc2.weight": (512, 512), "fc2.bias": (512,), "fc31.u_w": (256, 512),
            "fc31.sigma_w": (256, 512), "fc31.u_b": (256,), "fc32.weight": (128, 512), "fc41.u_w": (21, 256),
            "fc42.weight": (1, 128)}
    for k, s in want.items():
        assert tuple(p[k].shape) == s, k
    assert len(p) == 20
    # the reference's initialisers: sigma = 0.5 / sqrt(in), weight_norm = ||W||_F
    assert torch.allclose(p["fc31.sigma_w"], torch.full((256, 512), 0.5 / 512 ** 0.5))
    assert torch.allclose(p["fc2.weight_norm"], p["fc2.weight"].norm())
    assert tuple(random_direct_dqn(hidden2=512, noisy_layers=0)["fc31.weight"].shape) == (256, 512)
    # the narrow net is what it was
    q = random_direct_dqn(seed=3)
    assert tuple(q["fc2.weight"].shape) == (256, 512) and tuple(q["fc31.u_w"].shape) == (256, 256)
    with pytest.raises(ValueError, match="hidden2"):
        random_direct_dqn(hidden2=384)


def test_wide_forward_matches_per_row_restatement():
    """forward() with H2 = 512 against W = u + sigma o (eps_out eps_in^T) and F.linear, row by row."""
    p = _p64(hidden2=512)
    B = 128
    tr, _, nz = V.make_batch(B, 2, hidden2=512)
    assert nz.shape == (32, 1045) and V.noise_len(512) == 1045 and V.noise_len(256) == 789
    x = torch.as_tensor(tr[:, :5]).double()
    noise = torch.as_tensor(nz).double()
    q, m = V.forward(p, x, noise)
    wn = lambda n: p[f"{n}.weight"] * (p[f"{n}.weight_norm"] / p[f"{n}.weight"].norm())   # noqa: E731
    for b in (0, 3, 4, 77, 127):
        c = b // (B // 32)
        ei3, eo3, ei4, eo4 = noise[c, :512], noise[c, 512:768], noise[c, 768:1024], noise[c, 1024:]
        h1 = torch.relu(F.linear(x[b], wn("fc1"), p["fc1.bias"]))
        h2 = torch.relu(F.linear(h1, wn("fc2"), p["fc2.bias"]))
        assert h2.shape == (512,)
        W3 = p["fc31.u_w"] + p["fc31.sigma_w"] * torch.outer(eo3, ei3)
        a3 = torch.relu(F.linear(h2, W3, p["fc31.u_b"] + p["fc31.sigma_b"] * eo3))
        W4 = p["fc41.u_w"] + p["fc41.sigma_w"] * torch.outer(eo4, ei4)
        qb = F.linear(a3, W4, p["fc41.u_b"] + p["fc41.sigma_b"] * eo4)
        mb = F.linear(torch.relu(F.linear(h2, wn("fc32"), p["fc32.bias"])), wn("fc42"), p["fc42.bias"])
        np.testing.assert_allclose(q[b].numpy(), qb.numpy(), rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(m[b].item(), mb.item(), rtol=1e-11, atol=1e-12)
    # the actor's per-env form agrees with the chunked one where env b uses chunk b's noise
    qa = V.actor_q(p, x[:32].numpy(), nz)
    q32, _ = V.forward(p, x[:32], noise)
    np.testing.assert_allclose(qa, q32.numpy(), rtol=1e-11, atol=1e-12)


def test_three_targets_on_a_hand_computed_batch():
    nsv = torch.tensor([2.0, -1.0, 0.5, 4.0], dtype=torch.float64)
    g, alive, fail = 0.75, 10.0, -1.0
    r = torch.tensor([1.0, -1.0, 1.0, -1.0], dtype=torch.float64)
    y = V.td_target(nsv.clone(), r, "alive", g, alive, fail)
    np.testing.assert_allclose(y.numpy(), [1.5 + 2.5, 0.0, 0.375 + 2.5, 0.0], rtol=0, atol=1e-15)
    r = torch.tensor([-0.4, -1.0, -1.5, -0.999], dtype=torch.float64)   # above, equal, below, just above
    y = V.td_target(nsv.clone(), r, "reward_fail", g, alive, fail)
    np.testing.assert_allclose(y.numpy(), [1.5 - 0.1, -1.0, -1.5, 3.0 - 0.24975], rtol=0, atol=1e-15)
    y = V.td_target(nsv.clone(), r, "reward", g, alive, fail)
    np.testing.assert_allclose(y.numpy(), [1.5 - 0.1, -0.75 - 0.25, 0.375 - 0.375, 3.0 - 0.24975], rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        V.td_target(nsv, r, "other", g, alive, fail)


@pytest.mark.parametrize("target", V.TARGETS)
def test_td_loss_uses_the_target_and_the_batch_suits_it(target):
    """td_loss == (sav - td_target)^2 with sav, nsv from forward(); make_batch's reward column per mode."""
    p = _p64(hidden2=512)
    tr, w, nz = V.make_batch(128, 2, hidden2=512, target=target)
    r = tr[:, -1]
    if target == "alive":
        assert set(np.unique(r)) == {-1.0, 1.0}
    elif target == "reward_fail":
        assert (r == -1.0).sum() >= 3 and (r < -1.0).sum() >= 3 and ((r > -1.0) & (r < 0)).sum() >= 96
        assert 0.08 <= (r <= -1.0).mean() <= 0.25
    else:
        assert (r < 0).all() and np.unique(r).size > 100
    t = lambda a: torch.as_tensor(a).double()   # noqa: E731
    loss, ul, qn = V.td_loss(p, p, t(tr), t(w), t(nz), target=target, gamma=0.99)
    q, m = V.forward(p, t(tr[:, :5]), t(nz))
    qt, mt = V.forward(p, t(tr[:, 5:10]), t(nz))
    a = qt.argmax(1)
    nsv = qt[torch.arange(128), a] + mt - qt.mean(1)
    sav = q[torch.arange(128), torch.as_tensor(tr[:, -2]).long()] + m - q.mean(1)
    y = V.td_target(nsv, t(r), target, 0.99, 10.0, -1.0)
    np.testing.assert_allclose(ul.numpy(), ((sav - y) ** 2).numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(loss.item(), (ul * t(w)).mean().item(), rtol=1e-12)


def _fd_entries(f, x, idx, h=1e-6):
    """Central finite differences of the scalar f at entries idx of the fp64 tensor x (test_learner_cpu._fd)."""
    flat = x.view(-1)
    out = []
    for i in idx:
        old = flat[i].item()
        flat[i] = old + h
        up = f().item()
        flat[i] = old - h
        dn = f().item()
        flat[i] = old
        out.append((up - dn) / (2 * h))
    return np.array(out)


@pytest.mark.parametrize("target", V.TARGETS)
def test_wide_gradients_match_finite_differences(target):
    """Autograd through the wide restatement against central differences, a few entries per tensor, with
    test_learner_cpu.py's method and bound (h = 1e-6, rtol 1e-6, atol 1e-8)."""
    p = _p64(hidden2=512)
    tr, w, nz = V.make_batch(128, 2, hidden2=512, target=target)
    t = lambda a: torch.as_tensor(a).double()   # noqa: E731
    trt, wt, nzt = t(tr), t(w), t(nz)
    _, _, g, qn = V.loss_and_grads(p, p, tr, w, nz, target=target)
    # differences are meaningful only where no argmax flips under the perturbation
    assert V.clear_rows(qn).all()
    target_p = {k: v.clone() for k, v in p.items()}
    f = lambda: V.td_loss(p, target_p, trt, wt, nzt, target=target)[0]   # noqa: E731
    rng = np.random.default_rng(0)
    with torch.no_grad():
        for k, v in p.items():
            idx = rng.choice(v.numel(), size=min(3, v.numel()), replace=False)
            fd = _fd_entries(f, v, idx)
            np.testing.assert_allclose(g[k].reshape(-1)[idx], fd, rtol=1e-6, atol=1e-8, err_msg=k)


def test_dqn_params_struct_matches_header(tmp_path):
    """_lib.QcDqnParams mirrors the header's qc_dqn_params (offsets and size), and the QC_TD_* constants."""
    import shutil
    import subprocess
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "off.c"
    cls = _lib.QcDqnParams
    lines = [f'printf("%zu\\n", offsetof(qc_dqn_params, {n}));\n' for n, _ in cls._fields_]
    lines.append('printf("%zu\\n", sizeof(qc_dqn_params));\n')
    lines.append('printf("%d %d %d\\n", QC_TD_ALIVE, QC_TD_REWARD_FAIL, QC_TD_REWARD);\n')
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qcart.h"\nint main(void){\n' + "".join(lines)
                   + 'return 0;}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [getattr(cls, n).offset for n, _ in cls._fields_] + [ctypes.sizeof(cls)]
    want += [_lib.TD_TARGETS["alive"], _lib.TD_TARGETS["reward_fail"], _lib.TD_TARGETS["reward"]]
    assert got == want
    assert [n for n, _ in cls._fields_][-1] == "hidden2"
    assert [n for n, _ in _lib.QcLearnerParams._fields_][-4:] == ["hidden2", "target_mode", "beta1", "beta2"]
