"""Checker of the device measurement learner: a torch-on-CPU restatement of one update of the measurement-input
network, written from the equations, with gradients from autograd. Runs in fp64 (the reference of the parity
tests) and in fp32 (what rounding alone costs).

A replay row, K = L / m:  [meas (L + m, newest first) | forces (K + 1, newest first) | action | reward]
    next[0] = row[0 : L]           next[1][k m : (k + 1) m] = forces[k]
    prev[0] = row[m : m + L]       prev[1][k m : (k + 1) m] = forces[k + 1]          k = 0 .. K - 1
Network:
    y1 = relu(conv1 x)  Conv1d(2, 32, 13, stride 5);  y2 = relu(conv2 y1)  (32, 64, 11, 4);
    y3 = relu(conv3 y2)  (64, 64, 9, 4);  h1 = relu(fc1 flatten(y3))  Linear(64 T3, 256)
    a = relu(fc21 h1); Q = fc31 a          fc21, fc31 factorised noisy (learner_ref.noisy_linear)
    m = fc32 relu(fc22 h1)                 fc22, fc32 weight-normalised: W_eff = W g / ||W||_F
Loss: learner_ref.td_loss's double-DQN TD loss ("alive" target) on (Q, m).
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import learner_ref as R

CONV = ((2, 32, 13, 5), (32, 64, 11, 4), (64, 64, 9, 4))   # (in, out, kernel, stride)
CHUNKS = R.CHUNKS


def conv_len(n, k, s):
    return (n - k) // s + 1


def dims(L):
    t = [L]
    for _, _, k, s in CONV:
        t.append(conv_len(t[-1], k, s))
    return t


def row_len(L, m):
    return L + m + L // m + 3


def assemble(tr, L, m):
    """(next, prev) [B, 2, L] from rows [B, row_len] (tensor ops: differentiable w.r.t. nothing, pure copies)."""
    K = L // m
    forces = tr[:, L + m:L + m + K + 1]
    nxt = torch.stack([tr[:, 0:L], forces[:, 0:K].repeat_interleave(m, 1)], 1)
    prv = torch.stack([tr[:, m:m + L], forces[:, 1:K + 1].repeat_interleave(m, 1)], 1)
    return nxt, prv


def assemble_loop(tr, L, m):
    """The same, index by index (numpy)."""
    tr = np.asarray(tr)
    B, K = tr.shape[0], L // m
    nxt = np.zeros((B, 2, L), tr.dtype)
    prv = np.zeros((B, 2, L), tr.dtype)
    for b in range(B):
        for i in range(L):
            nxt[b, 0, i] = tr[b, i]
            prv[b, 0, i] = tr[b, m + i]
        for k in range(K):
            for r in range(m):
                nxt[b, 1, k * m + r] = tr[b, L + m + k]
                prv[b, 1, k * m + r] = tr[b, L + m + k + 1]
    return nxt, prv


def random_params(L, n_actions=21, seed=0):
    """DQN_measurement-shaped parameters with non-zero random conv and fc biases."""
    g = torch.Generator().manual_seed(seed)

    def uni(shape, bound):
        return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * bound

    p = {}
    for j, (ci, co, k, _) in enumerate(CONV):
        b = 1.0 / np.sqrt(ci * k)
        p[f"conv{j + 1}.weight"] = uni((co, ci, k), b)
        p[f"conv{j + 1}.bias"] = uni((co,), b)
    flat = 64 * dims(L)[3]
    p["fc1.weight"] = uni((256, flat), 1.0 / np.sqrt(flat))
    p["fc1.bias"] = uni((256,), 1.0 / np.sqrt(flat))
    for name, i, o in (("fc21", 256, 256), ("fc31", 256, n_actions)):
        s = 0.5 / np.sqrt(i)
        p[f"{name}.u_w"] = uni((o, i), np.sqrt(6.0 / i))
        p[f"{name}.sigma_w"] = torch.full((o, i), s, dtype=torch.float64)
        p[f"{name}.u_b"] = uni((o,), 0.05)
        p[f"{name}.sigma_b"] = torch.full((o,), s, dtype=torch.float64)
    for name, i, o in (("fc22", 256, 128), ("fc32", 128, 1)):
        w = uni((o, i), 1.0 / np.sqrt(i))
        p[f"{name}.weight"] = w
        p[f"{name}.bias"] = uni((o,), 1.0 / np.sqrt(i))
        p[f"{name}.weight_norm"] = w.norm() * 1.1
    return {k: v.to(torch.float32) for k, v in p.items()}


def make_batch(B, seed, L, m, n_actions=21, failing_reward=-1.0, fresh_rows=(1, 7, 40)):
    """Rows: a smooth signal plus noise as measurements, forces from the action grid, uniform actions, reward
    failing on ~15 % of the rows else 1, IS weights in [0.3, 1], noise f(randn(32, 789)). The rows in
    `fresh_rows` have the older part of their history exact zeros (a fresh episode's record)."""
    rng = np.random.default_rng(seed)
    K = L // m
    t = np.arange(L + m)
    meas = 0.6 * np.sin(0.02 * t[None, :] + rng.uniform(0, 6.28, (B, 1))) + 0.5 * rng.standard_normal((B, L + m))
    forces = (rng.integers(0, n_actions, (B, K + 1)) - n_actions // 2) * 0.2
    for n, b in enumerate(fresh_rows):
        if b < B:
            keep = (n + 1) * m            # only the newest `keep` measurements exist
            meas[b, keep:] = 0.0
            forces[b, n + 1:] = 0.0
    act = rng.integers(0, n_actions, B)
    rew = np.where(rng.random(B) < 0.15, failing_reward, 1.0)
    w = rng.uniform(0.3, 1.0, B)
    noise = R.f_noise(rng.standard_normal((CHUNKS, 3 * 256 + n_actions)))
    tr = np.concatenate([meas, forces, act[:, None].astype(np.float64), rew[:, None]], axis=1).astype(np.float32)
    assert tr.shape[1] == row_len(L, m)
    return tr, w.astype(np.float32), noise.astype(np.float32)


def features(p, x):
    """relu(fc1(flatten(conv stack))) [B, 256]; also the pre-activation conv outputs (tests)."""
    zs = []
    h = x
    for j, (_, _, _, s) in enumerate(CONV):
        z = F.conv1d(h, p[f"conv{j + 1}.weight"], p[f"conv{j + 1}.bias"], stride=s)
        zs.append(z)
        h = torch.relu(z)
    h1 = torch.relu(F.linear(h.flatten(1), p["fc1.weight"], p["fc1.bias"]))
    return h1, zs


def forward(p, x, noise):
    """(Q [B, A], m [B]) for x [B, 2, L] and noise [32, noise_len] (eps_in21, eps_out21, eps_in31, eps_out31)."""
    h1, _ = features(p, x)
    a = torch.relu(R.noisy_linear(p["fc21.u_w"], p["fc21.u_b"], p["fc21.sigma_w"], p["fc21.sigma_b"], h1,
                                  noise[:, 0:256], noise[:, 256:512]))
    q = R.noisy_linear(p["fc31.u_w"], p["fc31.u_b"], p["fc31.sigma_w"], p["fc31.sigma_b"], a,
                       noise[:, 512:768], noise[:, 768:])
    m = R._wn(p, "fc32", torch.relu(R._wn(p, "fc22", h1))).squeeze(1)
    return q, m


def td_loss(p, pt, tr, w, noise, L, m, gamma=0.998, alive_reward=10.0, failing_reward=-1.0):
    """(loss, ul [B], q_next_online [B, A])."""
    nxt, prv = assemble(tr, L, m)
    act = tr[:, -2].long()
    with torch.no_grad():
        qn, _ = forward(p, nxt, noise)
        a_star = qn.max(1)[1]
        qt, mt = forward(pt, nxt, noise)
        nsv = qt.gather(1, a_star[:, None]).squeeze(1) + mt - qt.mean(1)
        y = nsv * gamma + (1.0 - gamma) * alive_reward
        y[tr[:, -1] == failing_reward] = 0.0
    q, mm = forward(p, prv, noise)
    sav = q.gather(1, act[:, None]).squeeze(1) + mm - q.mean(1)
    ul = (sav - y) ** 2
    return (ul * w).mean(), ul, qn


def loss_and_grads(params, target, tr, w, noise, L, m, dtype=torch.float64, **kw):
    """ul [B], loss, {name: grad}, Q_online(next) — numpy arrays, computed in `dtype`."""
    p = {k: v.requires_grad_(True) for k, v in R.to_params(params, dtype).items()}
    pt = R.to_params(target, dtype)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)   # noqa: E731
    loss, ul, qn = td_loss(p, pt, t(tr), t(w), t(noise), L, m, **kw)
    loss.backward()
    return (ul.detach().numpy(), float(loss.detach()), {k: v.grad.numpy() for k, v in p.items()}, qn.numpy())


def run_updates(params, tr, w, noise, n, L, m, lr=4e-4, backup_period=50, dtype=torch.float64, **kw):
    """n updates on one fixed batch: (losses, final online parameters, final target parameters)."""
    opt = R.LaProp(params, lr=lr, dtype=dtype)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)   # noqa: E731
    tr_t, w_t, nz_t = t(tr), t(w), t(noise)
    target, losses, counter = None, [], 0
    for _ in range(n):
        if counter == 0:
            target = R.to_params(opt.p, dtype)
        counter = (counter + 1) % backup_period
        p = {k: v.clone().requires_grad_(True) for k, v in opt.p.items()}
        loss, _, _ = td_loss(p, target, tr_t, w_t, nz_t, L, m, **kw)
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step({k: v.grad for k, v in p.items()})
    return losses, opt.p, target


def r32_table(L, m, B, seed=3, pseed=5):
    """Per tensor: max|g32 - g64| / max|g64| of this restatement run in fp32 and in fp64 (what fp32 rounding
    alone costs; the gradient tolerance's r32)."""
    p = random_params(L, seed=pseed)
    tr, w, nz = make_batch(B, seed, L, m)
    _, _, g64, _ = loss_and_grads(p, p, tr, w, nz, L, m, torch.float64)
    _, _, g32, _ = loss_and_grads(p, p, tr, w, nz, L, m, torch.float32)
    return {k: float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in g64}


if __name__ == "__main__":   # python -m tests.mlearner_ref L m B
    import sys
    L_, m_, B_ = (int(a) for a in sys.argv[1:4])
    for k_, v_ in r32_table(L_, m_, B_).items():
        print(f'    "{k_}": {v_:.1e},')
