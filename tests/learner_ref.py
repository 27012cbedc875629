"""Checker of the device DQN learner: a torch-on-CPU restatement of one learner update, written from the
equations (direct_DQN with the chunked NoisyNet noise, the double-DQN TD loss, LaProp), with gradients from
autograd. Runs in fp64 (the reference of the parity tests) and in fp32 (what rounding alone costs).

    h1 = relu(fc1 x); h2 = relu(fc2 h1)            fc1, fc2, fc32, fc42 weight-normalised: W_eff = W g / ||W||_F
    a3 = relu(fc31 h2); Q = fc41 a3                fc31, fc41 factorised noisy
    m  = fc42 relu(fc32 h2)
Noisy layer, row b of chunk c (32 contiguous chunks of B / 32 rows, one (eps_in, eps_out) pair per chunk):
    y_b = u_w x_b + u_b + eps_out_c o (sigma_w (eps_in_c o x_b) + sigma_b)
"""
import numpy as np
import torch

SCALE = np.array([1.5, 1.5, 0.4, 0.4, 0.2])
CHUNKS = 32


def f_noise(z):
    return np.sign(z) * np.sqrt(np.abs(z))


def make_batch(B, seed, L=5, n_actions=21, failing_reward=-1.0):
    """The test batch: prev = randn * scale, next = prev + 0.1 randn * scale, uniform actions, reward
    failing on ~15 % of the rows else 1, IS weights in [0.3, 1], noise f(randn(32, 789))."""
    rng = np.random.default_rng(seed)
    scale = np.resize(SCALE, L)
    prev = rng.standard_normal((B, L)) * scale
    nxt = prev + 0.1 * rng.standard_normal((B, L)) * scale
    act = rng.integers(0, n_actions, B)
    rew = np.where(rng.random(B) < 0.15, failing_reward, 1.0)
    w = rng.uniform(0.3, 1.0, B)
    noise = f_noise(rng.standard_normal((CHUNKS, 2 * 256 + 256 + n_actions)))
    tr = np.concatenate([prev, nxt, act[:, None].astype(np.float64), rew[:, None]], axis=1).astype(np.float32)
    return tr, w.astype(np.float32), noise.astype(np.float32)


def to_params(p, dtype):
    return {k: v.detach().cpu().to(dtype).clone() for k, v in p.items()}


def _wn(p, name, x):
    w = p[f"{name}.weight"]
    return x @ (w * (p[f"{name}.weight_norm"] / w.norm())).T + p[f"{name}.bias"]


def noisy_linear(u_w, u_b, s_w, s_b, x, eps_in, eps_out):
    """x [B, in]; eps_in [32, in], eps_out [32, out]: chunk c = b // (B / 32)."""
    rep = x.shape[0] // CHUNKS
    ei = eps_in.repeat_interleave(rep, 0)
    eo = eps_out.repeat_interleave(rep, 0)
    return x @ u_w.T + u_b + eo * ((ei * x) @ s_w.T + s_b)


def forward(p, x, noise):
    """(Q [B, A], m [B]) for x [B, L] and noise [32, noise_len] (eps_in31, eps_out31, eps_in41, eps_out41)."""
    h1 = torch.relu(_wn(p, "fc1", x))
    h2 = torch.relu(_wn(p, "fc2", h1))
    a3 = torch.relu(noisy_linear(p["fc31.u_w"], p["fc31.u_b"], p["fc31.sigma_w"], p["fc31.sigma_b"], h2,
                                 noise[:, 0:256], noise[:, 256:512]))
    q = noisy_linear(p["fc41.u_w"], p["fc41.u_b"], p["fc41.sigma_w"], p["fc41.sigma_b"], a3,
                     noise[:, 512:768], noise[:, 768:])
    m = _wn(p, "fc42", torch.relu(_wn(p, "fc32", h2))).squeeze(1)
    return q, m


def td_loss(p, pt, tr, w, noise, gamma=0.998, alive_reward=10.0, failing_reward=-1.0):
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
        y = nsv * gamma + (1.0 - gamma) * alive_reward
        y[tr[:, -1] == failing_reward] = 0.0
    q, m = forward(p, prev, noise)
    sav = q.gather(1, act[:, None]).squeeze(1) + m - q.mean(1)
    ul = (sav - y) ** 2
    return (ul * w).mean(), ul, qn


def loss_and_grads(params, target, tr, w, noise, dtype=torch.float64, **kw):
    """ul [B], loss, {name: grad}, Q_online(next) — numpy arrays, computed in `dtype`."""
    p = {k: v.requires_grad_(True) for k, v in to_params(params, dtype).items()}
    pt = to_params(target, dtype)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)   # noqa: E731
    loss, ul, qn = td_loss(p, pt, t(tr), t(w), t(noise), **kw)
    loss.backward()
    return (ul.detach().numpy(), float(loss.detach()), {k: v.grad.numpy() for k, v in p.items()}, qn.numpy())


class LaProp:
    """LaProp, centered, no amsgrad, no weight decay: per element
        v = v b2 + (1 - b2) g^2;  mu = mu b2 + (1 - b2) g;  den = v - mu^2 if step > 10 else v
        den = sqrt(den / l2) + eps;  e = e b1 + (1 - b1) lr g / den;  p -= e / (l1 / lr)   (divisor 1 at lr = 0)
    with the scalars step += 1, l1 = l1 b1 + (1 - b1) lr, l2 = l2 b2 + (1 - b2) updated first."""

    def __init__(self, params, lr=4e-4, betas=(0.9, 0.9995), eps=1e-15, dtype=torch.float64):
        self.p = to_params(params, dtype)
        self.lr, self.b1, self.b2, self.eps = lr, betas[0], betas[1], eps
        self.step_count, self.l1, self.l2 = 0, 0.0, 0.0
        self.e = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.mu = {k: torch.zeros_like(v) for k, v in self.p.items()}

    def step(self, grads):
        self.step_count += 1
        b1, b2, lr = self.b1, self.b2, self.lr
        self.l1 = self.l1 * b1 + (1 - b1) * lr
        self.l2 = self.l2 * b2 + (1 - b2)
        div = self.l1 / lr if lr != 0.0 else 1.0
        for k, p in self.p.items():
            g = torch.as_tensor(np.asarray(grads[k])).to(p.dtype).reshape(p.shape)
            v = self.v[k].mul_(b2).add_((1 - b2) * g * g)
            mu = self.mu[k].mul_(b2).add_((1 - b2) * g)
            den = v - mu * mu if self.step_count > 10 else v
            den = (den / self.l2).sqrt() + self.eps
            e = self.e[k].mul_(b1).add_((1 - b1) * lr * (g / den))
            p.sub_(e / div)


def run_updates(params, tr, w, noise, n, lr=4e-4, backup_period=50, dtype=torch.float32, **kw):
    """n updates on one fixed batch; the losses."""
    opt = LaProp(params, lr=lr, dtype=dtype)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)   # noqa: E731
    tr_t, w_t, nz_t = t(tr), t(w), t(noise)
    target, losses, counter = None, [], 0
    for _ in range(n):
        if counter == 0:
            target = to_params(opt.p, dtype)
        counter = (counter + 1) % backup_period
        p = {k: v.clone().requires_grad_(True) for k, v in opt.p.items()}
        loss, _, _ = td_loss(p, target, tr_t, w_t, nz_t, **kw)
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step({k: v.grad for k, v in p.items()})
    return losses
