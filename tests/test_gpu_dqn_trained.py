"""GPU: the device DQN actors and DQNLearner on "trained-like" parameters and with a target net that differs from
the online net, against the fp64 restatements (tests/dqn_variants_ref.py, oracle/dqn.py) on identical parameters,
inputs and noise.

random_direct_dqn uses the reference's initialisers: weight_norm = ||W||_F (so the weight-norm scale g / ||W|| is 1
in every forward, and in the backward's chain rule), u_b = 0, one sigma per layer. dqn_variants_ref.trained_like
moves the parameters off all three, as the first optimizer step does. And DQNLearner's other parity tests call the
restatement with target = online, where double DQN is a plain max: here the learner runs 7 updates across two
target refreshes, and every update is compared with the restatement on the learner's own online and target
parameters. tests/test_dqn_trained_cpu.py shows, on the restatement alone, that these inputs see the mistakes in
question by more than 100 tolerances.

Tolerances are the project's (test_gpu_actor.py, test_gpu_learner.py, test_gpu_dqn_variants.py, test_gpu_mactor.py):
  * action values: <= 2e-5 max|q| + 1e-5 (the measurement actor: 5e-5 max|q| + 1e-5); actions equal wherever the
    top-two gap exceeds twice that;
  * per-sample losses: <= 2e-5 max|ul_ref| + 1e-5, on rows whose top-two gap of Q_online(next) exceeds twice the q
    tolerance (a borderline argmax changes a target and says nothing about the kernel); the scalar loss too when
    every row is clear;
  * gradients, per tensor, when every row is clear: <= max(2e-5, 8 r32) max|g_ref|;
  * LaProp: <= 1e-5 lr + 2^-23 |p|, one step from the learner's own parameters on its own gradients.
r32 is the restatement in fp32 against fp64 on the CPU (never the device), per tensor the largest value along the
restatement's own 7 updates (`python -m tests.dqn_variants_ref HIDDEN2 TARGET`, or `HIDDEN2 N_ACTIONS DATA_LENGTH`
for the last two rows; the per-tensor values
are dqn_variants_ref.DRIVERS / HEADS, and test_dqn_trained_cpu.py measures them again). Largest over the 20 tensors:

    case (B = 128)                 update 1   2         3         4         5         6         7         losses
    256, alive        L 5  A 21    2.1e-6     5.7e-6    8.4e-6    1.5e-6    2.1e-6    9.6e-5    2.0e-6    0.06
    512, alive        L 5  A 21    2.8e-6     2.7e-6    2.5e-6    2.1e-6    2.3e-6    1.1e-5    2.2e-6    0.09
    512, reward_fail  L 5  A 21    4.2e-6     5.8e-6    3.1e-6    4.2e-6    1.7e-5    1.7e-5    5.0e-6    0.07
    256, reward       L 5  A 21    1.0e-5     1.9e-6    2.7e-6    1.6e-6    1.7e-6    6.0e-6    1.7e-6    0.06
    512, alive        L 9  A 32    2.6e-6                                                                  0.11
    256, alive        L 14 A 9     1.5e-6                                                                  0.03

(losses: max|ul32 - ul64| as a share of the ul tolerance; within 1/8, so that tolerance stays as it is). The values
above 2.5e-6 belong to the weight_norm gradients of fc1 / fc2 (9.6e-5, 5.9e-5 at update 6 of the first case), a
difference of two nearly equal sums, and to the mean branch fc32 / fc42, whose gradient is a signed sum of the
rows' errors that cancels as the loss falls; every other tensor stays at 2e-5.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import dqn  # noqa: E402
from tests import dqn_variants_ref as V  # noqa: E402
from tests.test_gpu_dqn_variants import check_actions, check_params, check_q, cuda, host  # noqa: E402
from tests.test_gpu_mactor import check as check_mq, make_records  # noqa: E402
from deepreinforcementlearningcontrolofquantumcartpoles_amd.actor import (DQNActor, MeasurementActor,  # noqa: E402
                                                                          random_direct_dqn,
                                                                          random_dqn_measurement)
from deepreinforcementlearningcontrolofquantumcartpoles_amd.learner import DQNLearner  # noqa: E402

LR = 4e-4
B = 128


def on_device(p):
    return {k: v.cuda() for k, v in p.items()}


# ---- 1. the actors ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy_layers", [2, 1, 0])
@pytest.mark.parametrize("hidden2", [256, 512])
def test_actor_on_trained_like_weights(hidden2, noisy_layers):
    """B = 100: three full 32-env tiles and a tail of 4."""
    p = V.trained_like(random_direct_dqn(noisy_layers=noisy_layers, seed=11, hidden2=hidden2), 3)
    actor = DQNActor(on_device(p), max_batch=100, seed=3)
    assert actor.hidden2 == hidden2 and actor.noise_len == V.noise_len(hidden2)
    obs, noise = V.actor_inputs(100, actor.noise_len)
    act, ex = actor.act(cuda(obs), noise=cuda(noise), want_q=True, want_random=True)
    q_ref = V.actor_q(p, obs, noise if noisy_layers else None)
    check_actions(act.cpu().numpy(), q_ref, check_q(ex["q"].cpu().numpy(), q_ref))
    assert int(ex["random"].sum()) == 0
    if (hidden2, noisy_layers) != (256, 2):
        return
    # a second trained-like set through load(): the prepared weights are replaced, scale and all
    p2 = V.trained_like(random_direct_dqn(seed=16), 4)
    q2_ref = V.actor_q(p2, obs, noise)
    assert np.abs(q2_ref - q_ref).max() > 100 * V.q_tol(q2_ref)
    actor.load(on_device(p2))
    act, ex = actor.act(cuda(obs), noise=cuda(noise), want_q=True)
    check_actions(act.cpu().numpy(), q2_ref, check_q(ex["q"].cpu().numpy(), q2_ref))


def test_measurement_actor_smallest_awkward_geometry():
    """L = 500: T = 98 / 22 / 4, every convolution with uncovered trailing inputs (remainders 2 / 3 / 1) and a fc1
    of 256 inputs, where one missed position is far above the tolerance. B = 37 in chunks of 16 (two full chunks and
    a tail of 5 at env 32) with max_batch = 48: the buffers' leading dimension is not B. Non-zero conv biases,
    fc21 / fc31 trained-like."""
    L, nb = 500, 37
    p = random_dqn_measurement(read_length=L, seed=21)
    g = torch.Generator().manual_seed(1)
    for j in (1, 2, 3):
        p[f"conv{j}.bias"] = torch.randn(p[f"conv{j}.bias"].shape, generator=g) * 0.1
    p = V.trained_like(p, 3)
    assert (p["fc21.u_b"] != 0).all() and p["fc31.sigma_w"].unique().numel() > 1000
    obs = make_records(nb, L, seed=nb)
    noise = dqn.f_noise(np.random.default_rng(2).standard_normal((nb, 789))).astype(np.float32)
    q_ref = dqn.forward_measurement(p, obs.astype(np.float64), noise.astype(np.float64))
    srt = np.sort(q_ref, axis=1)
    assert ((srt[:, -1] - srt[:, -2]) > 2 * (5e-5 * np.abs(q_ref).max() + 1e-5)).all()   # every row clear
    actor = MeasurementActor(on_device(p), read_length=L, max_batch=48, seed=3, chunk=16)
    assert actor.flat_len == 256 and actor.noise_len == 789
    act, ex = actor.act(cuda(obs), noise=cuda(noise), want_q=True, want_random=True)
    rel = check_mq(ex["q"].cpu().numpy(), q_ref, act.cpu().numpy())
    print(f"max|q err| / max|q| {rel:.2e}")
    assert int(ex["random"].sum()) == 0


# ---- 2. one learner update against the restatement on given online and target parameters ------------------------
def check_update(learner, opt, before, target_p, batch, dev_batch, r32, what, **kw):
    """One update of `learner`, whose online parameters are `before` and whose target net must be `target_p` (None:
    refreshed from `before` by this update). Losses, gradients and the LaProp step by the module docstring's rules.
    Returns (the target parameters, whether every row was clear)."""
    refresh = target_p is None
    ul = learner.update(dev_batch[0], dev_batch[1], noise=dev_batch[2]).cpu().double().numpy()
    loss = float(learner.last_loss.cpu())
    tgt = host(learner.state_dict(target=True))
    if refresh:
        target_p = before
    for k in tgt:
        assert torch.equal(tgt[k], target_p[k]), (what, k, "target")
    g_dev = host(learner.grads())
    after = host(learner.state_dict())
    ul_ref, loss_ref, g_ref, qn = V.loss_and_grads(before, target_p, *batch, **kw)
    clear = V.clear_rows(qn)
    tol = 2e-5 * np.abs(ul_ref).max() + 1e-5
    err = np.abs(ul - ul_ref)[clear].max()
    print(f"{what}: clear rows {clear.mean():.3f}, max|ul err| {err:.3e} (tol {tol:.3e})")
    assert clear.mean() >= 0.9
    assert err <= tol, (what, err, tol)
    if clear.all():
        assert abs(loss - loss_ref) <= tol, (what, loss, loss_ref)
        assert set(g_dev) == set(g_ref) and len(g_ref) == 20
        bad = []
        for k, r in g_ref.items():
            bound = V.grad_bound(r32, k)
            e = np.abs(g_dev[k].double().numpy() - r).max() / np.abs(r).max()
            print(f"    {k:17s} max|g| {np.abs(r).max():.3e} err {e:.2e} rel (bound {bound:.2e})")
            if not e <= bound:
                bad.append((k, e, bound))
        assert not bad, (what, bad)
    # LaProp from `before` on the device's own gradients; the fp64 e, v, mu carry on
    opt.p = V.to_params(before, torch.float64)
    opt.step({k: v.double() for k, v in g_dev.items()})
    check_params(after, opt.p, LR, what)
    assert learner.stats()["launches_per_update"] == (10 if refresh else 8), what
    return target_p, bool(clear.all())


@pytest.mark.parametrize("hidden2,target", list(V.DRIVERS))
def test_learner_across_target_refreshes(hidden2, target):
    """The four drivers' learners (learner.py's table), 7 updates with backup_period 3 on two alternating batches:
    updates 1, 4 and 7 refresh the target, the four between them run on a stale one. After every update the
    target is, bitwise, the online net that the last refreshing update started from (state_dict(target=True) is
    the raw copy), and the losses and gradients are the restatement's for that pair, so the prepared target copy
    that the kernels read is the same net. The gradient comparison needs every row's argmax clear; the restatement's
    own trajectory has that at all 7 updates (test_dqn_trained_cpu.py), the device's must have it at a stale update
    of each period at least."""
    d = V.DRIVERS[(hidden2, target)]
    p0 = V.trained_like(random_direct_dqn(seed=11, hidden2=hidden2), 3)
    batches = [V.make_batch(B, s, hidden2=hidden2, target=target) for s in d["seeds"]]
    dev = [tuple(cuda(a) for a in bt) for bt in batches]
    learner = DQNLearner(p0, batch_size=B, lr=LR, backup_period=3, target=target, betas=d["betas"])
    assert learner.hidden2 == hidden2
    opt = V.LaProp(p0, lr=LR, betas=d["betas"])
    target_p, full = None, []
    for n in range(7):
        before = host(learner.state_dict())
        if n == 0:
            assert all(torch.equal(before[k], p0[k]) for k in p0)
        target_p, clear = check_update(learner, opt, before, None if n % 3 == 0 else target_p, batches[n % 2],
                                       dev[n % 2], d["r32"], f"H2 {hidden2} {target} update {n + 1}", target=target)
        assert any(not torch.equal(target_p[k], host(learner.state_dict())[k]) for k in target_p)
        full.append(clear)
    print("updates with every row clear:", full)
    assert full[0] and (full[1] or full[2]) and (full[4] or full[5])
    st = learner.stats()
    assert st["updates"] == 7 and st["step"] == 7 and st["backup_counter"] == 7 % 3 and st["nonfinite"] == 0
    if (hidden2, target) != (512, "reward_fail"):
        return
    # push: the actor's q is the restatement's for the learner's online parameters (and no longer p0's)
    online = host(learner.state_dict())
    actor = DQNActor(on_device(p0), max_batch=100, seed=3)
    learner.push(actor)
    obs, noise = V.actor_inputs(100, actor.noise_len)
    act, ex = actor.act(cuda(obs), noise=cuda(noise), want_q=True)
    q_ref = V.actor_q(online, obs, noise)
    assert np.abs(q_ref - V.actor_q(p0, obs, noise)).max() > 100 * V.q_tol(q_ref)
    check_actions(act.cpu().numpy(), q_ref, check_q(ex["q"].cpu().numpy(), q_ref))


@pytest.mark.parametrize("case", list(V.HEADS), ids=lambda c: "H{}-A{}-L{}".format(*c))
def test_learner_other_head_widths(case):
    """n_actions = 32 (the maximum: no padded Q rows) at data_length 9, and n_actions = 9 at data_length 14: one
    update on trained-like weights, with the checks above. Every row is clear and every action present
    (test_dqn_trained_cpu.py)."""
    hidden2, A, L = case
    d = V.HEADS[case]
    p0 = V.trained_like(random_direct_dqn(data_length=L, n_actions=A, seed=11, hidden2=hidden2), 3)
    batch = V.make_batch(B, d["seed"], L=L, n_actions=A, hidden2=hidden2)
    learner = DQNLearner(p0, batch_size=B, lr=LR)
    assert (learner.n_actions, learner.data_length, learner.noise_len) == (A, L, hidden2 + 512 + A)
    opt = V.LaProp(p0, lr=LR)
    _, clear = check_update(learner, opt, host(learner.state_dict()), None, batch, tuple(cuda(a) for a in batch),
                            d["r32"], f"H2 {hidden2} A {A} L {L}")
    assert clear
    st = learner.stats()
    assert st["updates"] == 1 and st["step"] == 1 and st["nonfinite"] == 0
