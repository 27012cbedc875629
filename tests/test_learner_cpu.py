"""CPU: the learner's checker (tests/learner_ref.py) against finite differences and LaProp's closed forms, and
the loud failure of qc_learner_create without a GPU."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import learner_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deepreinforcementlearningcontrolofquantumcartpoles_amd", "libqcart.so")


def _fd(f, x, h=1e-6):
    """Central finite differences of the scalar f at the fp64 tensor x."""
    g = torch.zeros_like(x)
    flat, gf = x.view(-1), g.view(-1)
    for i in range(flat.numel()):
        old = flat[i].item()
        flat[i] = old + h
        up = f().item()
        flat[i] = old - h
        dn = f().item()
        flat[i] = old
        gf[i] = (up - dn) / (2 * h)
    return g


def test_weight_norm_gradient_matches_finite_differences():
    """dg = <G, W> / ||W||, dW = (g / ||W||)(G - <G, W> W / ||W||^2) with G = dY X^T, against central
    differences of the restatement's weight-normalised layer in fp64."""
    g = torch.Generator().manual_seed(1)
    W = torch.randn(6, 5, generator=g, dtype=torch.float64)
    b = torch.randn(6, generator=g, dtype=torch.float64)
    gn = torch.tensor(1.7, dtype=torch.float64)
    x = torch.randn(8, 5, generator=g, dtype=torch.float64)
    c = torch.randn(8, 6, generator=g, dtype=torch.float64)
    p = {"l.weight": W, "l.bias": b, "l.weight_norm": gn}
    f = lambda: (R._wn(p, "l", x) * c).sum()   # noqa: E731
    G = c.T @ x
    n = W.norm()
    dot = (G * W).sum()
    dW = (gn / n) * (G - dot * W / n ** 2)
    np.testing.assert_allclose(dW.numpy(), _fd(f, W).numpy(), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose((dot / n).item(), _fd(f, gn.view(1)).item(), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(c.sum(0).numpy(), _fd(f, b).numpy(), rtol=1e-6, atol=1e-8)
    # and autograd agrees with the closed form
    W.requires_grad_(True)
    f().backward()
    np.testing.assert_allclose(W.grad.numpy(), dW.numpy(), rtol=1e-10, atol=1e-12)


def test_noisy_layer_gradient_matches_finite_differences():
    """du_w = dY X^T, dsigma_w = (eps_out o dY)(eps_in o X)^T, du_b = sum dY, dsigma_b = sum eps_out o dY,
    dX = u_w^T dY + eps_in o (sigma_w^T (eps_out o dY)), per chunk, against central differences in fp64."""
    g = torch.Generator().manual_seed(2)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    B, I, O = 64, 4, 3
    u_w, s_w, u_b, s_b = rn(O, I), rn(O, I), rn(O), rn(O)
    x, c = rn(B, I), rn(B, O)
    ei, eo = rn(32, I), rn(32, O)
    f = lambda: (R.noisy_linear(u_w, u_b, s_w, s_b, x, ei, eo) * c).sum()   # noqa: E731
    rep = B // 32
    eir, eor = ei.repeat_interleave(rep, 0), eo.repeat_interleave(rep, 0)
    want = {
        "u_w": c.T @ x, "s_w": (eor * c).T @ (eir * x), "u_b": c.sum(0), "s_b": (eor * c).sum(0),
        "x": c @ u_w + eir * ((eor * c) @ s_w),
    }
    for name, t in (("u_w", u_w), ("s_w", s_w), ("u_b", u_b), ("s_b", s_b), ("x", x)):
        np.testing.assert_allclose(want[name].numpy(), _fd(f, t).numpy(), rtol=1e-6, atol=1e-8, err_msg=name)


def test_restatement_rounding_fp32_against_fp64():
    """What fp32 rounding alone costs on the test batch (the device tests' tolerances sit about 10x above)."""
    from deepreinforcementlearningcontrolofquantumcartpoles_amd.actor import random_direct_dqn
    p = random_direct_dqn(seed=11)
    tr, w, nz = R.make_batch(128, 2)
    ul64, l64, g64, _ = R.loss_and_grads(p, p, tr, w, nz, torch.float64)
    ul32, l32, g32, _ = R.loss_and_grads(p, p, tr, w, nz, torch.float32)
    assert len(g64) == 20
    assert np.abs(ul32 - ul64).max() <= 2e-5 * np.abs(ul64).max() + 1e-5
    for k in g64:
        assert np.abs(g32[k] - g64[k]).max() <= 2e-5 * np.abs(g64[k]).max(), k


def test_laprop_first_step_is_minus_lr_sign():
    g = torch.Generator().manual_seed(3)
    p = {"a": torch.randn(50, generator=g, dtype=torch.float64)}
    grad = {"a": torch.randn(50, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-6, 3, (50,), generator=g)}
    opt = R.LaProp(p, lr=4e-4)
    opt.step(grad)
    np.testing.assert_allclose((opt.p["a"] - p["a"]).numpy(), -4e-4 * np.sign(grad["a"].numpy()), rtol=1e-6)


def test_laprop_centred_term_switches_on_at_step_11():
    """With a constant gradient, den = v through step 10 (the update stays lr sign(g) in the limit) and
    v - mu^2 from step 11: the step-11 increment of e follows the centred denominator."""
    p = {"a": torch.zeros(3, dtype=torch.float64)}
    grad = {"a": torch.tensor([0.5, -2.0, 1e-3], dtype=torch.float64)}
    opt = R.LaProp(p, lr=1e-3)
    b1, b2 = 0.9, 0.9995
    for step in range(1, 13):
        e_old = opt.e["a"].clone()
        opt.step(grad)
        inc = (opt.e["a"] - b1 * e_old) / ((1 - b1) * 1e-3)      # g / den of this step
        v, mu, l2 = opt.v["a"], opt.mu["a"], opt.l2
        plain, centred = grad["a"] / (v / l2).sqrt(), grad["a"] / ((v - mu * mu) / l2).sqrt()
        want = plain if step <= 10 else centred
        np.testing.assert_allclose(inc.numpy(), want.numpy(), rtol=1e-9)
        assert not np.allclose(plain.numpy(), centred.numpy(), rtol=1e-4)
    # lr = 0: divisor 1, parameters unchanged
    opt0 = R.LaProp(p, lr=0.0)
    opt0.step(grad)
    np.testing.assert_array_equal(opt0.p["a"].numpy(), p["a"].numpy())


@pytest.mark.skipif(not os.path.exists(LIB), reason="libqcart.so not built")
def test_learner_create_without_gpu_fails_loudly():
    """No CPU fallback: without a HIP device qc_learner_create returns an error and no handle."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
    p = _lib.QcLearnerParams()
    p.data_length, p.n_actions, p.batch_size, p.backup_period = 5, 21, 128, 300
    p.gamma, p.lr, p.alive_reward, p.failing_reward = 0.998, 4e-4, 10.0, -1.0
    h = ctypes.c_void_p()
    rc = _lib.lib().qc_learner_create(ctypes.byref(p), 0, ctypes.byref(h))
    assert rc < 0 and not h.value
    assert b"HIP" in _lib.lib().qc_learner_last_error(None)
    # the batch sizes of the reference's per-row noise branch are refused before the device is touched
    p.batch_size = 100
    assert _lib.lib().qc_learner_create(ctypes.byref(p), 0, ctypes.byref(h)) == -1
    assert b"multiple of 128" in _lib.lib().qc_learner_last_error(None)


def test_learner_params_struct_matches_header(tmp_path):
    """_lib.QcLearnerParams / QcLearnerStats mirror the header's structs (offsets and sizes)."""
    import shutil
    import subprocess
    from deepreinforcementlearningcontrolofquantumcartpoles_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "off.c"
    lines = []
    for cname, cls in (("qc_learner_params", _lib.QcLearnerParams), ("qc_learner_stats_t", _lib.QcLearnerStats)):
        lines += [f'printf("%zu\\n", offsetof({cname}, {n}));\n' for n, _ in cls._fields_]
        lines.append(f'printf("%zu\\n", sizeof({cname}));\n')
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qcart.h"\nint main(void){\n' + "".join(lines)
                   + 'return 0;}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for cls in (_lib.QcLearnerParams, _lib.QcLearnerStats):
        want += [getattr(cls, n).offset for n, _ in cls._fields_] + [ctypes.sizeof(cls)]
    assert got == want
