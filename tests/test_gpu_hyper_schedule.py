"""GPU: the learner's hyper-parameters in device memory (include/cat_ppo.h: cat_ppo_loss_grad_dev, cat_ppo_adam_step_dev,
cat_ppo_schedule_step) and the scheduled trainer (``RoleConfig.lr_schedule``).  Everything is compared bit for bit (``torch.equal`` /
equal bit patterns): the _dev entries against their by-value twins called with the numbers the block holds, the schedule kernel against the
NumPy restatement of tests/test_hyper_schedule_host.py, a replayed graph against eager steps at the learning rate the block held at the
time, and the trainer's learning rates against the restatement."""
import numpy as np
import pytest

from tests.test_hyper_schedule_host import (ANNEAL_CASES, ANNEAL_PAIRS, KL_ARGS, KL_COUNT, KL_SUM, LR, SCHED_ANNEAL, SCHED_KL, STRIDE, F, _bits,
                                            kl_table, np_schedule)

pytestmark = pytest.mark.gpu


def _block(rows):
    """hyper fp32 [G, 8] on the device from (lr, entropy scale, ratio clip) rows; the rest 0"""
    import torch
    h = torch.zeros(len(rows), STRIDE, device="cuda")
    h[:, :3] = torch.tensor(rows, dtype=torch.float32)
    return h


# ---------------------------------------------------------------------------------------------- the loss
def test_loss_from_the_block_equals_the_by_value_loss():
    import torch
    from as_cops_and_thieves_amd import _learn_native as ln
    G, M = 3, 2 * 256 + 37                      # a partly filled block of 256 and more than one chunk of the 64
    gen = torch.Generator(device="cuda").manual_seed(11)
    logits = (2.0 * torch.randn(G, M, 4, generator=gen, device="cuda")).to(torch.bfloat16)
    values = torch.randn(G, M, generator=gen, device="cuda").to(torch.bfloat16)
    act = torch.randint(0, 4, (G, M), generator=gen, device="cuda")
    ret = torch.randn(G, M, generator=gen, device="cuda")
    adv = torch.randn(G, M, generator=gen, device="cuda")
    logp = torch.log_softmax(logits.float(), -1).gather(-1, act.unsqueeze(-1)).squeeze(-1)
    old = logp + 0.25 * torch.randn(G, M, generator=gen, device="cuda")                 # ratios on both sides of every clip range below
    data = (logits, values, act, old, adv, ret)
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    want = ln.ppo_loss_grad(*data, 0.15, 0.5, 0.02)
    got = ln.ppo_loss_grad_dev(*data, _block([(7.0, 0.02, 0.15)] * G), 0.5)             # (the learning rate's word is not the loss's)
    torch.cuda.synchronize()
    assert same(got, want) and got[0].shape == (G, 4) and float(want[1].float().abs().max()) > 0
    rows = [(1e-4, 0.02, 0.15), (3e-4, 0.0, 0.3), (1e-3, 0.05, 0.05)]
    got = ln.ppo_loss_grad_dev(*data, _block(rows), 0.5)
    for g, (_, entropy, clip) in enumerate(rows):
        want = ln.ppo_loss_grad(*data, clip, 0.5, entropy)
        torch.cuda.synchronize()
        assert all(torch.equal(x[g], y[g]) for x, y in zip(got, want)), g
    assert not torch.equal(ln.ppo_loss_grad(*data, 0.3, 0.5, 0.0)[1][0], got[1][0])     # the rows' numbers do change the gradient


# ---------------------------------------------------------------------------------------------- the optimiser step
class _Adam:
    """One optimiser state on the device; ``step`` by value or from a block."""
    B1, B2, EPS, CLIP, THRESHOLD = 0.9, 0.999, 1e-8, 0.5, 0.015

    def __init__(self, G, P, seed):
        import torch
        gen = torch.Generator(device="cuda").manual_seed(seed)
        f = dict(device="cuda", dtype=torch.float32)
        self.master = torch.randn(G, P, generator=gen, **f)
        self.col = (torch.rand(G, P, generator=gen, **f) > 0.3).float()
        self.m, self.v, self.steps = torch.zeros(G, P, **f), torch.zeros(G, P, **f), torch.zeros(G, P, **f)
        self.active, self.kl_out, self.scratch = torch.ones(G, **f), torch.zeros(G, **f), torch.zeros(G, 256, **f)
        self.lp = torch.zeros(G, P, device="cuda", dtype=torch.bfloat16)

    def tensors(self):
        return {k: getattr(self, k) for k in ("master", "m", "v", "steps", "lp", "active", "kl_out")}

    def step(self, ar, lr=None, hyper=None):
        from as_cops_and_thieves_amd import _learn_native as ln
        head = (ar, self.col, self.active, self.m, self.v, self.steps, self.master, self.lp, self.kl_out, self.scratch)
        tail = (self.B1, self.B2, self.EPS, self.CLIP, self.THRESHOLD)
        if hyper is None:
            ln.ppo_adam_step(*head, lr, *tail)
        else:
            ln.ppo_adam_step_dev(*head, hyper, *tail)

    def clone(self):
        import copy
        other = copy.copy(self)
        for k, v in vars(self).items():
            setattr(other, k, v.clone())
        return other


def _gradients(G, P, seed):
    """three steps' fp32 [G, P + 1] gradient | KL buffers; agent 1 trips the KL gate (0.015) at the second"""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for step in range(3):
        ar = torch.randn(G, P + 1, generator=gen, device="cuda") * (0.001 if step == 2 else 1.0)       # the last: norm below the clip
        ar[:, -1] = torch.tensor([0.001 + 0.0007 * step, 0.02 if step == 1 else 0.002, 0.003 + 0.0011 * step], device="cuda")
        out.append(ar)
    return out


def test_adam_step_from_the_block_equals_the_by_value_step_and_sums_the_kl():
    import torch
    G, P, lr = 3, 1000, 1e-3
    plain = _Adam(G, P, seed=3)
    dev = plain.clone()
    hyper = _block([(lr, 0.02, 0.15)] * G)
    entered = []
    for k, ar in enumerate(_gradients(G, P, seed=4)):
        entered.append(dev.active.cpu().clone())
        plain.step(ar, lr=lr)
        dev.step(ar, hyper=hyper)
        torch.cuda.synchronize()
        for name, t in plain.tensors().items():
            assert torch.equal(t, dev.tensors()[name]), (k, name)
        assert torch.equal(dev.kl_out, ar[:, -1])
    assert dev.active.tolist() == [1.0, 0.0, 1.0] and float(dev.steps.max()) == 3.0
    assert [e.tolist() for e in entered] == [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 0.0, 1.0]]
    # the KL of every call an agent ENTERED active, added up in fp32 in call order: the tripping minibatch counts, the gated one does not
    want_sum, want_count = torch.zeros(G), torch.zeros(G)
    for e, ar in zip(entered, _gradients(G, P, seed=4)):
        want_sum = want_sum + torch.where(e != 0, ar[:, -1].cpu(), torch.zeros(G))
        want_count = want_count + (e != 0).float()
    assert torch.equal(hyper[:, KL_SUM].cpu(), want_sum) and torch.equal(hyper[:, KL_COUNT].cpu(), want_count)
    assert want_count.tolist() == [3.0, 2.0, 3.0]
    assert torch.equal(hyper[:, :3], _block([(lr, 0.02, 0.15)] * G)[:, :3]) and not hyper[:, 5:].any()


def test_adam_step_takes_every_agents_own_learning_rate():
    import torch
    G, P = 3, 1000
    rates = (1e-3, 3e-4, 5e-2)
    start = _Adam(G, P, seed=5)
    dev = start.clone()
    hyper = _block([(r, 0.0, 0.0) for r in rates])
    ars = _gradients(G, P, seed=6)
    for ar in ars:
        dev.step(ar, hyper=hyper)
    for g, r in enumerate(rates):
        plain = start.clone()
        for ar in ars:
            plain.step(ar, lr=r)
        torch.cuda.synchronize()
        for name, t in plain.tensors().items():
            assert torch.equal(t[g], dev.tensors()[name][g]), (g, name)
    assert not torch.equal(dev.master[0] - start.master[0], dev.master[2] - start.master[2])


# ---------------------------------------------------------------------------------------------- the schedule kernel
def test_schedule_kernel_kl_rule_equals_the_restatement():
    import torch
    from as_cops_and_thieves_amd import _learn_native as ln
    h0, active = kl_table()
    hyper = torch.from_numpy(h0.copy()).cuda()
    ln.ppo_schedule_step(hyper, torch.from_numpy(active).cuda(), SCHED_KL, **KL_ARGS)
    torch.cuda.synchronize()
    want = np_schedule(h0, active, SCHED_KL, **KL_ARGS)
    assert np.array_equal(_bits(hyper.cpu().numpy()), _bits(want)), (hyper, want)
    # fewer agents than the table: the rows beyond G are not the kernel's
    hyper = torch.from_numpy(h0.copy()).cuda()
    ln.ppo_schedule_step(hyper[:3], torch.from_numpy(active[:3].copy()).cuda(), SCHED_KL, **KL_ARGS)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(hyper[:3].cpu().numpy()), _bits(want[:3])) and np.array_equal(_bits(hyper[3:].cpu().numpy()), _bits(h0[3:]))


@pytest.mark.parametrize("mask,progress", ANNEAL_CASES)
def test_schedule_kernel_anneal_equals_the_restatement(mask, progress):
    import torch
    from as_cops_and_thieves_amd import _learn_native as ln
    h0, active = kl_table()
    for mode in (SCHED_ANNEAL, SCHED_ANNEAL | SCHED_KL):
        hyper = torch.from_numpy(h0.copy()).cuda()
        ln.ppo_schedule_step(hyper, torch.from_numpy(active).cuda(), mode, anneal_mask=mask, progress=progress, **ANNEAL_PAIRS, **KL_ARGS)
        torch.cuda.synchronize()
        want = np_schedule(h0, active, mode, anneal_mask=mask, progress=progress, **ANNEAL_PAIRS, **KL_ARGS)
        assert np.array_equal(_bits(hyper.cpu().numpy()), _bits(want)), (mode, hyper, want)


# ---------------------------------------------------------------------------------------------- a captured step follows the block
def test_a_replayed_graph_reads_the_learning_rate_the_block_holds_then():
    import torch
    G, P = 3, 1000
    rates = (1e-3, 4e-5)
    start = _Adam(G, P, seed=7)
    dev = start.clone()
    ar = _gradients(G, P, seed=8)[0]
    hyper = _block([(rates[0], 0.0, 0.0)] * G)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):               # once outside the capture: the code object is loaded
        dev.step(ar, hyper=hyper)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.step(ar, hyper=hyper)
    for name, t in start.tensors().items():     # what the warm-up and the capture moved goes back
        dev.tensors()[name].copy_(t)
    hyper[:, KL_SUM:].zero_()
    plain = start.clone()
    for k, r in enumerate(rates):
        hyper[:, LR] = r                        # a device write between replays; the graph object stays
        graph.replay()
        plain.step(ar, lr=r)
        torch.cuda.synchronize()
        for name, t in plain.tensors().items():
            assert torch.equal(t, dev.tensors()[name]), (k, name)
    assert hyper[:, KL_COUNT].tolist() == [2.0] * G
    other = start.clone()                       # ... and the second replay did not train at the first rate
    for _ in rates:
        other.step(ar, lr=rates[0])
    torch.cuda.synchronize()
    assert not torch.equal(other.master, dev.master)


# ---------------------------------------------------------------------------------------------- the trainer
EPOCHS, UPDATES = 2, 2


def _trainer(**rc_kw):
    from as_cops_and_thieves_amd.environments import VecCopsEnv
    from as_cops_and_thieves_amd.maps import load_preset
    from as_cops_and_thieves_amd.selfplay.mappo import MAPPOTrainer, RoleConfig, TrainerConfig
    rc = RoleConfig(learning_epochs=EPOCHS, mini_batches=2, random_timesteps=0, learning_starts=0, **rc_kw)
    env = VecCopsEnv(load_preset("squarinth"), 32, num_rays=64, max_step_count=60, seed=5)
    tc = TrainerConfig(horizon=16, policy_freeze_duration=0, opponent_freeze_duration=0, graph_update=True)
    return env, MAPPOTrainer(env, {"cop": rc, "thief": rc}, tc, seed=0)


def test_trainer_with_schedules_on_the_device():
    import torch
    digests = {}
    for name, kw in (("plain", {}), ("twin", {"lr_schedule": "kl_adaptive", "lr_factor": 1.0}), ("shrink", {"lr_schedule": "kl_adaptive", "lr_kl_target": 1e-12})):
        env, tr = _trainer(**kw)
        (rl,) = tr.roles.values()
        assert rl.native and rl.scheduled == (name != "plain") and hasattr(rl, "hyper") == (name != "plain")
        tr.collect(); tr.update()
        torch.cuda.synchronize()
        graphs = rl._graphs
        assert graphs, "the minibatch step was not captured"
        first = tr.read_stats()
        tr.collect(); tr.update()
        torch.cuda.synchronize()
        assert rl._graphs is graphs                                 # no recapture, whatever the block went through
        stats = tr.read_stats()
        digests[name] = tr.param_digest()
        if name != "plain":
            assert rl.hyper.is_cuda and rl.sched_active.tolist() == [1.0] * rl.G and not rl.hyper[:, 3:].any()
        if name == "twin":
            assert [stats[f"lr/{a}"] for a in tr.agents] == [float(F(1e-4))] * len(tr.agents)
        if name == "shrink":        # every epoch's mean KL is above 2e-12: EPOCHS shrink steps per update, by the restatement
            want = [_rate(EPOCHS * k) for k in (1, 2)]
            assert [first[f"lr/{a}"] for a in tr.agents] == [want[0]] * len(tr.agents)
            assert [stats[f"lr/{a}"] for a in tr.agents] == [want[1]] * len(tr.agents) and want[1] < want[0] < 1e-4
            assert all(stats[f"entropy_scale/{a}"] == float(F(0.02)) and stats[f"ratio_clip/{a}"] == float(F(0.15)) for a in tr.agents)
        env.check_errors(); env.close()
    assert digests["twin"] == digests["plain"] and digests["shrink"] != digests["plain"]


def _rate(steps):
    """fp32(1e-4), RoleConfig's learning rate, after ``steps`` shrink steps of the KL rule (the host file's restatement)"""
    h = np.zeros((1, STRIDE), np.float32)
    h[0, LR] = 1e-4
    for _ in range(steps):
        h[0, KL_SUM], h[0, KL_COUNT] = 1.0, 1.0
        h = np_schedule(h, np.ones(1, np.float32), SCHED_KL, **dict(KL_ARGS, kl_target=1e-12))
    return float(h[0, LR])
