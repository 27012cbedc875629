"""GPU: the device DQN learner (csrc/qcart_learner.hip through DQNLearner) against the torch-on-CPU
restatement tests/learner_ref.py on identical parameters, batches and noise.

Tolerances. The kernels compute in fp32 with exact-f32 MFMA accumulation, the restatement in fp64:
  * per-sample losses: <= 2e-5 max|ul| + 1e-5 (the actor test's fp32-MFMA tolerance, test_gpu_actor.py:25-30),
    on rows whose top-two gap of Q_online(next) exceeds twice that tolerance (a borderline argmax changes a
    target and says nothing about the kernel);
  * gradients, per tensor: <= 2e-5 max|g_ref| (fp32 rounding alone measures 2.5e-6 in the restatement);
  * LaProp: <= 1e-5 lr + 2^-23 |p| (a ten-operation fp32 chain on an update of size <= lr, plus one rounding
    of p), against the fp64 restatement on the same fp32 gradients.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import learner_ref as R  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd._lib import QCartError  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.actor import DQNActor, random_direct_dqn  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.learner import DQNLearner  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.replay import PrioritizedReplay  # noqa: E402

LR = 4e-4


def cuda(x):
    return torch.as_tensor(np.asarray(x)).cuda()


def host(d):
    return {k: v.detach().cpu() for k, v in d.items()}


def make(p, B, seed, L=5, **kw):
    tr, w, nz = R.make_batch(B, seed, L=L)
    return DQNLearner(p, batch_size=B, **kw), tr, w, nz


def check_params(dev, ref, lr, what=""):
    for k, r in ref.items():
        r = r.numpy()
        err = np.abs(dev[k].double().numpy() - r)
        tol = 1e-5 * lr + 2.0 ** -23 * np.abs(r)
        assert (err <= tol).all(), (what, k, float((err - tol).max()), float(err.max()))


def top_two_gap(q):
    s = np.sort(q, axis=1)
    return s[:, -1] - s[:, -2]


# ---- 1. loss parity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(128, 5), (512, 5), (128, 20)])
def test_loss_matches_restatement(B, L):
    p = random_direct_dqn(data_length=L, seed=11)
    learner, tr, w, nz = make(p, B, 2, L=L, lr=LR)
    ul = learner.update(cuda(tr), cuda(w), noise=cuda(nz)).cpu().numpy()
    ul_ref, loss_ref, _, qn = R.loss_and_grads(p, p, tr, w, nz)
    tol = 2e-5 * np.abs(ul_ref).max() + 1e-5
    qtol = 2e-5 * np.abs(qn).max() + 1e-5
    clear = top_two_gap(qn) > 2 * qtol
    err = np.abs(ul - ul_ref)[clear].max()
    print(f"B={B} L={L}: clear rows {clear.mean():.3f}, max|ul err| {err:.3e} (tol {tol:.3e})")
    assert clear.mean() >= 0.9
    assert err <= tol, (err, tol)
    if clear.all():
        assert abs(float(learner.last_loss.cpu()) - loss_ref) <= tol
    st = learner.stats()
    assert st["updates"] == 1 and st["step"] == 1 and st["nonfinite"] == 0
    print("launches per update (first update, with the target copy):", st["launches_per_update"])


# ---- 2. gradient parity -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,seed", [(128, 5, 2), (512, 5, 3), (128, 20, 2)])
def test_gradients_match_fp64_autograd(B, L, seed):
    p = random_direct_dqn(data_length=L, seed=11)
    tr, w, nz = R.make_batch(B, seed, L=L)
    ul_ref, _, g_ref, qn = R.loss_and_grads(p, p, tr, w, nz)
    # the precondition, on the restatement: every row's argmax is clear, and the batch has fail rows,
    # non-uniform weights and every action
    assert (top_two_gap(qn) > 2 * (2e-5 * np.abs(qn).max() + 1e-5)).all()
    assert (tr[:, -1] == -1).any() and (tr[:, -1] == 1).any() and np.unique(w).size > B // 2
    assert set(tr[:, -2].astype(int)) == set(range(21))
    learner = DQNLearner(p, batch_size=B, lr=LR)
    learner.update(cuda(tr), cuda(w), noise=cuda(nz))
    g = host(learner.grads())
    assert set(g) == set(g_ref) and len(g) == 20
    bad = []
    for k, r in g_ref.items():
        err = np.abs(g[k].double().numpy() - r).max()
        tol = 2e-5 * np.abs(r).max()
        print(f"{k:14s} max|g| {np.abs(r).max():.3e} err {err:.3e} ({err / np.abs(r).max():.2e} rel)")
        if not err <= tol:
            bad.append((k, err, tol))
    assert not bad, bad


# ---- 3. optimizer -----------------------------------------------------------------------------------------
def test_laprop_on_injected_gradients():
    p = random_direct_dqn(seed=11)
    learner = DQNLearner(p, batch_size=128, lr=LR)
    ref = R.LaProp(p, lr=LR)
    gen = torch.Generator().manual_seed(5)
    lr = LR
    for step in range(1, 13):        # crosses the centred switch (step 11)
        if step == 6:
            lr = 1e-4
            learner.set_lr(lr)
            ref.lr = lr
        if step == 9:                # lr = 0: divisor 1, e still decays
            lr = 0.0
            learner.set_lr(lr)
            ref.lr = lr
        if step == 10:
            lr = LR
            learner.set_lr(lr)
            ref.lr = lr
        grads = {k: torch.randn(v.shape, generator=gen) * 10.0 ** float(torch.randint(-4, 1, (1,), generator=gen))
                 for k, v in p.items()}
        learner.apply({k: v.cuda() for k, v in grads.items()})
        ref.step(grads)
        dev = host(learner.state_dict())
        # at lr = 0 the update is the decaying e, of the size of the lr that built it (1e-4)
        check_params(dev, ref.p, lr if lr > 0 else 1e-4, f"step {step}")
        # the bound is one step's: the next step starts from the device's parameters (the fp64 e, v, mu carry on)
        ref.p = {k: v.double() for k, v in dev.items()}
    st = learner.stats()
    assert st["step"] == 12 and abs(st["l1"] - ref.l1) < 1e-15 and abs(st["l2"] - ref.l2) < 1e-15


# ---- 4. the update composes the two -------------------------------------------------------------------------
def test_update_is_laprop_on_its_own_gradients():
    p = random_direct_dqn(seed=11)
    learner, tr, w, nz = make(p, 128, 2, lr=LR)
    learner.update(cuda(tr), cuda(w), noise=cuda(nz))
    ref = R.LaProp(p, lr=LR)
    ref.step(host(learner.grads()))
    check_params(host(learner.state_dict()), ref.p, LR)


# ---- 5. target schedule -----------------------------------------------------------------------------------
def test_target_follows_every_backup_period():
    p = random_direct_dqn(seed=11)
    learner, tr, w, nz = make(p, 128, 2, lr=LR, backup_period=3)
    snaps = []
    for _ in range(4):
        learner.update(cuda(tr), cuda(w), noise=cuda(nz))
        snaps.append(host(learner.state_dict()))
    tgt = host(learner.state_dict(target=True))
    assert learner.stats()["backup_counter"] == 1
    for k in tgt:
        assert torch.equal(tgt[k], snaps[2][k]), k          # copied at the start of update 4
    assert any(not torch.equal(tgt[k], snaps[3][k]) for k in tgt)


# ---- 6. determinism and keyed noise -----------------------------------------------------------------------
def test_bit_identical_runs_and_keyed_noise():
    p = random_direct_dqn(seed=11)
    tr, w, nz = R.make_batch(128, 2)
    ends = []
    for _ in range(2):
        learner = DQNLearner(p, batch_size=128, lr=LR, seed=7)
        for _ in range(5):
            learner.update(cuda(tr), cuda(w), noise=cuda(nz))
        ends.append(host(learner.state_dict()))
    for k in ends[0]:
        assert torch.equal(ends[0][k], ends[1][k]), k
    uls = []
    for counter in (3, 3, 4):
        learner = DQNLearner(p, batch_size=128, lr=LR, seed=7)
        uls.append(learner.update(cuda(tr), cuda(w), counter=counter).cpu())
    assert torch.equal(uls[0], uls[1])
    assert not torch.equal(uls[0], uls[2])
    assert torch.isfinite(uls[0]).all()


# ---- 7. it learns -----------------------------------------------------------------------------------------
def test_fixed_batch_loss_falls():
    p = random_direct_dqn(seed=11)
    tr, w, nz = R.make_batch(128, 2)
    ref = R.run_updates(p, tr, w, nz, 200, lr=LR, backup_period=50)
    assert np.mean(ref[-10:]) <= 0.05 * ref[0], (ref[0], np.mean(ref[-10:]))
    learner = DQNLearner(p, batch_size=128, lr=LR, backup_period=50)
    trc, wc, nzc = cuda(tr), cuda(w), cuda(nz)
    losses = []
    for _ in range(200):
        learner.update(trc, wc, noise=nzc)
        losses.append(learner.last_loss.clone())
    losses = torch.cat(losses).cpu().numpy()
    print(f"first loss {losses[0]:.4e} (restatement {ref[0]:.4e}), last 10 mean {losses[-10:].mean():.4e} "
          f"(restatement {np.mean(ref[-10:]):.4e})")
    assert losses[-10:].mean() <= 0.05 * losses[0]
    assert learner.stats()["nonfinite"] == 0


# ---- 8. wiring --------------------------------------------------------------------------------------------
def test_step_with_replay_and_push_to_actor():
    p = random_direct_dqn(seed=11)
    B = 128
    learner = DQNLearner(p, batch_size=B, lr=LR, seed=1)
    tr, _, _ = R.make_batch(4 * B, 4)
    mem, twin = (PrioritizedReplay(1024, 12, policy="sequential", seed=9) for _ in range(2))
    for m in (mem, twin):
        m.store(cuda(tr[:100]))
    assert learner.step(mem) is None                  # len(memory) < batch_size
    for m in (mem, twin):
        m.store(cuda(tr[100:]))
    before = mem.buffers()[0].clone()
    ul = learner.step(mem, counter=0)
    assert ul is not None and ul.shape == (B,)
    idx, w, rows = twin.obtain_sample(B)              # the same Philox stream: the same sample
    ul2 = DQNLearner(p, batch_size=B, lr=LR, seed=1).update(rows, w, counter=0)
    assert torch.equal(ul, ul2)
    twin.batch_update(idx, ul2)
    assert torch.equal(mem.buffers()[0], twin.buffers()[0])
    assert not torch.equal(mem.buffers()[0], before)

    actor = DQNActor({k: v.cuda() for k, v in p.items()}, max_batch=256, seed=3)
    learner.push(actor)
    fresh = DQNActor(learner.state_dict(), max_batch=256, seed=3)
    obs = cuda(tr[:256, :5].copy())
    a1, e1 = actor.act(obs, noisy=False, want_q=True)
    a2, e2 = fresh.act(obs, noisy=False, want_q=True)
    assert torch.equal(e1["q"], e2["q"]) and torch.equal(a1, a2)
    stale = DQNActor({k: v.cuda() for k, v in p.items()}, max_batch=256, seed=3)
    assert not torch.equal(stale.act(obs, noisy=False, want_q=True)[1]["q"], e1["q"])


# ---- 9. refusals ------------------------------------------------------------------------------------------
def test_refusals():
    p = random_direct_dqn(seed=11)
    with pytest.raises(ValueError):
        DQNLearner(p, batch_size=100)
    learner, tr, w, nz = make(p, 128, 2, lr=LR)
    with pytest.raises(ValueError):
        learner.update(cuda(tr[:, :11]), cuda(w))
    with pytest.raises(ValueError):
        learner.update(cuda(tr[:64]), cuda(w[:64]))
    bad = tr.copy()
    bad[5, -2] = 21.0
    learner.update(cuda(bad), cuda(w), noise=cuda(nz))      # clamped on the device ...
    with pytest.raises(QCartError, match="action"):        # ... and reported, as qc_step's actions are
        learner.stats()
    assert learner.stats()["updates"] == 1                   # reported once
