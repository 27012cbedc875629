"""Checker of the device measurement learner and actor on the harmonic driver's net: tests/mlearner_ref.py's
torch-on-CPU restatement with weight-normalised convolutions and the TD target as an argument, written from the
equations, gradients from autograd.

    conv_n's effective weight   W_n g_n / ||W_n||_F      one scalar g_n per layer, ||.||_F over the whole [CO][CI][KS]
    the rest of the network     tests/mlearner_ref.py    (fc1 plain, fc21 / fc31 factorised noisy, fc22 / fc32
                                                          weight-normalised)
    the TD target               tests/dqn_variants_ref.td_target: "alive", "reward_fail" or "reward"

effective(p) forms the effective conv weights inside the autograd graph, so the gradients of conv_n.weight and
conv_n.weight_norm are autograd's; a parameter dict without conv_n.weight_norm keys passes through unchanged (the
plain stack). The two mistakes a device path can make, acting on the raw W (the weight_norm dropped) or on W g
(the norm not divided out), are `mistake="raw"` / `"no_norm"`, for the tests that show they are visible.

    python -m tests.mlearner_wn_ref L m B      the r32 table of the gradient tolerance (fp32 against fp64, CPU)
"""
import numpy as np
import torch

from tests import dqn_variants_ref as V
from tests import mlearner_ref as M
from tests.learner_ref import LaProp, to_params

CONV_NAMES = ("conv1", "conv2", "conv3")


def effective(p, mistake=None):
    """p with every weight-normalised convolution's weight replaced by W g / ||W||_F (differentiable)."""
    out = dict(p)
    for name in CONV_NAMES:
        if f"{name}.weight_norm" not in p:
            continue
        w, g = p[f"{name}.weight"], p[f"{name}.weight_norm"]
        if mistake == "raw":
            out[f"{name}.weight"] = w
        elif mistake == "no_norm":
            out[f"{name}.weight"] = w * g
        else:
            out[f"{name}.weight"] = w * (g / w.norm())
    return out


def random_params(L, seed=0, conv_weight_norm=True, n_actions=21):
    """mlearner_ref.random_params (non-zero conv and fc biases) and, per convolution, weight_norm = ||W||_F times
    its own factor in [0.7, 1.4] (dqn_variants_ref.trained_like's rule: no scale g / ||W|| is 1, no two are equal)."""
    p = M.random_params(L, n_actions=n_actions, seed=seed)
    if conv_weight_norm:
        g = torch.Generator().manual_seed(1000 + seed)
        for name in CONV_NAMES:
            f = 0.7 + 0.7 * torch.rand((), generator=g, dtype=torch.float64)
            p[f"{name}.weight_norm"] = (p[f"{name}.weight"].double().norm() * f).to(torch.float32)
    return p


def make_batch(B, seed, L, m, target="alive", failing_reward=-1.0):
    """mlearner_ref.make_batch's rows, weights and noise; the reward column is the target's
    (dqn_variants_ref.make_batch): "alive" 1 / failing_reward, "reward_fail" reals in (failing_reward, 0) with
    ~15 % at or below failing_reward, "reward" negative reals."""
    tr, w, nz = M.make_batch(B, seed, L, m, failing_reward=failing_reward)
    if target != "alive":
        rng = np.random.default_rng(7000 + seed)
        u, v = rng.random(B), rng.random(B)
        if target == "reward_fail":
            rew = failing_reward * (0.02 + 0.96 * v)
            fail = np.flatnonzero(u < 0.15)
            rew[fail[0::2]] = failing_reward
            rew[fail[1::2]] = failing_reward * (1.0 + v[fail[1::2]])
        elif target == "reward":
            rew = -2.0 * np.abs(failing_reward) * (0.01 + v)
        else:
            raise ValueError(target)
        tr = tr.copy()
        tr[:, -1] = rew.astype(np.float32)
    return tr, w, nz


def forward(p, x, noise, mistake=None):
    """(Q [B, A], m [B]) with chunk noise [32, noise_len]."""
    return M.forward(effective(p, mistake), x, noise)


def actor_q(params, obs, dtype=torch.float64, mistake=None):
    """The actor's mean-weight action values [B, A] (numpy; noisy = 0) for obs [B, 2, L]."""
    p = effective(to_params(params, dtype), mistake)
    h1, _ = M.features(p, torch.as_tensor(np.asarray(obs)).to(dtype))
    a = torch.relu(h1 @ p["fc21.u_w"].T + p["fc21.u_b"])
    return (a @ p["fc31.u_w"].T + p["fc31.u_b"]).numpy()


def td_loss(p, pt, tr, w, noise, L, m, target="alive", gamma=0.998, alive_reward=10.0, failing_reward=-1.0,
            mistake=None):
    """(loss, ul [B], q_next_online [B, A]); p's tensors may require grad."""
    nxt, prv = M.assemble(tr, L, m)
    act = tr[:, -2].long()
    with torch.no_grad():
        qn, _ = forward(p, nxt, noise, mistake)
        a_star = qn.max(1)[1]
        qt, mt = forward(pt, nxt, noise, mistake)
        nsv = qt.gather(1, a_star[:, None]).squeeze(1) + mt - qt.mean(1)
        y = V.td_target(nsv, tr[:, -1], target, gamma, alive_reward, failing_reward)
    q, mm = forward(p, prv, noise, mistake)
    sav = q.gather(1, act[:, None]).squeeze(1) + mm - q.mean(1)
    ul = (sav - y) ** 2
    return (ul * w).mean(), ul, qn


def loss_and_grads(params, target_params, tr, w, noise, L, m, dtype=torch.float64, **kw):
    """ul [B], loss, {name: grad}, Q_online(next) — numpy arrays, computed in `dtype`."""
    p = {k: v.requires_grad_(True) for k, v in to_params(params, dtype).items()}
    pt = to_params(target_params, dtype)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)   # noqa: E731
    loss, ul, qn = td_loss(p, pt, t(tr), t(w), t(noise), L, m, **kw)
    loss.backward()
    return (ul.detach().numpy(), float(loss.detach()), {k: v.grad.numpy() for k, v in p.items()}, qn.numpy())


def run_updates(params, tr, w, noise, n, L, m, lr=4e-4, betas=(0.9, 0.9995), backup_period=50, dtype=torch.float64,
                **kw):
    """n updates on one fixed batch: (losses, final online parameters, final target parameters)."""
    opt = LaProp(params, lr=lr, betas=betas, dtype=dtype)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)   # noqa: E731
    tr_t, w_t, nz_t = t(tr), t(w), t(noise)
    tgt, losses, counter = None, [], 0
    for _ in range(n):
        if counter == 0:
            tgt = to_params(opt.p, dtype)
        counter = (counter + 1) % backup_period
        p = {k: v.clone().requires_grad_(True) for k, v in opt.p.items()}
        loss, _, _ = td_loss(p, tgt, tr_t, w_t, nz_t, L, m, **kw)
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step({k: v.grad for k, v in p.items()})
    return losses, opt.p, tgt


def r32_table(L, m, B, seed=2, pseed=5, target="reward"):
    """Per tensor: max|g32 - g64| / max|g64| of this restatement run in fp32 and in fp64 on
    random_params(L, pseed) and make_batch(B, seed, L, m, target) (what fp32 rounding alone costs)."""
    p = random_params(L, seed=pseed)
    tr, w, nz = make_batch(B, seed, L, m, target)
    _, _, g64, _ = loss_and_grads(p, p, tr, w, nz, L, m, torch.float64, target=target)
    _, _, g32, _ = loss_and_grads(p, p, tr, w, nz, L, m, torch.float32, target=target)
    return {k: float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in g64}


if __name__ == "__main__":   # python -m tests.mlearner_wn_ref L m B [target]
    import sys
    L_, m_, B_ = (int(a) for a in sys.argv[1:4])
    for k_, v_ in r32_table(L_, m_, B_, target=sys.argv[4] if len(sys.argv) > 4 else "reward").items():
        print(f'    "{k_}": {v_:.1e},')
