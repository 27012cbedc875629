"""Checker of the per-driver variants of the device DQN actor and learner: tests/learner_ref.py's torch-on-CPU
restatement with fc2's width H2 as an argument and the three TD targets, written from the equations.

    h1 = relu(fc1 x); h2 = relu(fc2 h1)            h2: [B, H2], H2 = 256 or 512
    a3 = relu(fc31 h2); Q = fc41 a3                fc31 (H2 -> 256), fc41 (256 -> A) factorised noisy
    m  = fc42 relu(fc32 h2)                        fc32 (H2 -> 128)
One noise sample: eps_in31 [H2], eps_out31 [256], eps_in41 [256], eps_out41 [A]  (H2 + 512 + A floats).
TD target of a row with reward r, nsv the target net's value of the online net's argmax action:
    "alive"        y = gamma nsv + (1 - gamma) alive_reward;  y = 0 where r == failing_reward
    "reward_fail"  y = gamma nsv + (1 - gamma) r;             y = r where r <= failing_reward
    "reward"       y = gamma nsv + (1 - gamma) r
"""
import numpy as np
import torch

from tests.learner_ref import CHUNKS, SCALE, LaProp, _wn, f_noise, noisy_linear, to_params  # noqa: F401

TARGETS = ("alive", "reward_fail", "reward")


def noise_len(hidden2, n_actions=21):
    return hidden2 + 512 + n_actions


def noise_slices(noise, hidden2):
    """(eps_in31, eps_out31, eps_in41, eps_out41) of noise [n, noise_len]."""
    h = hidden2
    return noise[:, 0:h], noise[:, h:h + 256], noise[:, h + 256:h + 512], noise[:, h + 512:]


def hidden2_of(p):
    return p["fc2.weight"].shape[0]


def forward(p, x, noise):
    """(Q [B, A], m [B]) for x [B, L] and chunk noise [32, noise_len]; H2 is fc2.weight's."""
    ei3, eo3, ei4, eo4 = noise_slices(noise, hidden2_of(p))
    h1 = torch.relu(_wn(p, "fc1", x))
    h2 = torch.relu(_wn(p, "fc2", h1))
    a3 = torch.relu(noisy_linear(p["fc31.u_w"], p["fc31.u_b"], p["fc31.sigma_w"], p["fc31.sigma_b"], h2, ei3, eo3))
    q = noisy_linear(p["fc41.u_w"], p["fc41.u_b"], p["fc41.sigma_w"], p["fc41.sigma_b"], a3, ei4, eo4)
    m = _wn(p, "fc42", torch.relu(_wn(p, "fc32", h2))).squeeze(1)
    return q, m


def _layer(p, name, x, ei, eo):
    """One of fc31 / fc41, factorised noisy (per-row noise ei [B, in], eo [B, out]; None: the mean weights) or
    weight-normalised."""
    if f"{name}.u_w" not in p:
        return _wn(p, name, x)
    y = x @ p[f"{name}.u_w"].T + p[f"{name}.u_b"]
    if ei is not None:
        y = y + eo * ((ei * x) @ p[f"{name}.sigma_w"].T + p[f"{name}.sigma_b"])
    return y


def actor_q(params, obs, noise=None, dtype=torch.float64):
    """The actor's action values [B, A] (numpy) for obs [B, L] and per-env noise [B, noise_len] (None: the mean
    weights); any noisy_layers."""
    p = to_params(params, dtype)
    x = torch.as_tensor(np.asarray(obs)).to(dtype)
    sl = (None,) * 4
    if noise is not None:
        sl = noise_slices(torch.as_tensor(np.asarray(noise)).to(dtype), hidden2_of(p))
    h2 = torch.relu(_wn(p, "fc2", torch.relu(_wn(p, "fc1", x))))
    a3 = torch.relu(_layer(p, "fc31", h2, sl[0], sl[1]))
    return _layer(p, "fc41", a3, sl[2], sl[3]).numpy()


def td_target(nsv, r, target, gamma, alive_reward, failing_reward):
    if target == "alive":
        y = nsv * gamma + (1.0 - gamma) * alive_reward
        y[r == failing_reward] = 0.0
    elif target == "reward_fail":
        y = nsv * gamma + (1.0 - gamma) * r
        fail = r <= failing_reward
        y[fail] = r[fail]
    elif target == "reward":
        y = nsv * gamma + (1.0 - gamma) * r
    else:
        raise ValueError(target)
    return y


def td_loss(p, pt, tr, w, noise, target="alive", gamma=0.998, alive_reward=10.0, failing_reward=-1.0):
    """(loss, ul [B], q_next_online [B, A]) of the online parameters p and target parameters pt; p's tensors
    may require grad. tr, w, noise: tensors of p's dtype."""
    L = (tr.shape[1] - 2) // 2
    prev, nxt = tr[:, :L], tr[:, L:2 * L]
    act = tr[:, -2].long()
    with torch.no_grad():
        qn, _ = forward(p, nxt, noise)
        a_star = qn.max(1)[1]
        qt, mt = forward(pt, nxt, noise)
        nsv = qt.gather(1, a_star[:, None]).squeeze(1) + mt - qt.mean(1)
        y = td_target(nsv, tr[:, -1], target, gamma, alive_reward, failing_reward)
    q, m = forward(p, prev, noise)
    sav = q.gather(1, act[:, None]).squeeze(1) + m - q.mean(1)
    ul = (sav - y) ** 2
    return (ul * w).mean(), ul, qn


def loss_and_grads(params, target_params, tr, w, noise, dtype=torch.float64, **kw):
    """ul [B], loss, {name: grad}, Q_online(next) — numpy arrays, computed in `dtype`."""
    p = {k: v.requires_grad_(True) for k, v in to_params(params, dtype).items()}
    pt = to_params(target_params, dtype)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)   # noqa: E731
    loss, ul, qn = td_loss(p, pt, t(tr), t(w), t(noise), **kw)
    loss.backward()
    return (ul.detach().numpy(), float(loss.detach()), {k: v.grad.numpy() for k, v in p.items()}, qn.numpy())


def make_batch(B, seed, L=5, n_actions=21, hidden2=256, target="alive", failing_reward=-1.0):
    """learner_ref.make_batch's states, actions and weights, noise f(randn(32, noise_len(hidden2))), and a reward
    column for the target: "alive" 1 / failing_reward (~15 %); "reward_fail" reals in (failing_reward, 0) with
    ~15 % of the rows at or below failing_reward, alternately equal to it and strictly below; "reward" negative
    reals (some below failing_reward: it has no meaning there)."""
    rng = np.random.default_rng(seed)
    scale = np.resize(SCALE, L)
    prev = rng.standard_normal((B, L)) * scale
    nxt = prev + 0.1 * rng.standard_normal((B, L)) * scale
    act = rng.integers(0, n_actions, B)
    u, v = rng.random(B), rng.random(B)
    if target == "alive":
        rew = np.where(u < 0.15, failing_reward, 1.0)
    elif target == "reward_fail":
        rew = failing_reward * (0.02 + 0.96 * v)                     # inside (failing_reward, 0)
        fail = np.flatnonzero(u < 0.15)
        rew[fail[0::2]] = failing_reward                             # equal: == and <= agree
        rew[fail[1::2]] = failing_reward * (1.0 + v[fail[1::2]])     # strictly below: only <= catches them
    elif target == "reward":
        rew = -2.0 * np.abs(failing_reward) * (0.01 + v)
    else:
        raise ValueError(target)
    w = rng.uniform(0.3, 1.0, B)
    noise = f_noise(rng.standard_normal((CHUNKS, noise_len(hidden2, n_actions))))
    tr = np.concatenate([prev, nxt, act[:, None].astype(np.float64), rew[:, None]], axis=1).astype(np.float32)
    return tr, w.astype(np.float32), noise.astype(np.float32)


def top_two_gap(q):
    s = np.sort(q, axis=1)
    return s[:, -1] - s[:, -2]


def q_tol(q):
    """The project's fp32-MFMA tolerance on action values (test_gpu_actor.py)."""
    return 2e-5 * np.abs(q).max() + 1e-5


def clear_rows(qn):
    """Rows whose argmax of Q_online(next) is not borderline: top-two gap above twice the q tolerance."""
    return top_two_gap(qn) > 2 * q_tol(qn)
