"""The GPU steps of tests/test_gpu_act_step.py, one per process: ``python -m tests.act_steps STEP``.  A step prints its figures and
exits 0 when every check holds, 1 with the failed checks listed otherwise."""
from __future__ import annotations

import json
import sys
import tempfile
from pathlib import Path

import torch

FAILED = []


def check(ok, what):
    if not bool(ok):
        FAILED.append(what)
        print("FAILED:", what, flush=True)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def make(roster, N, R, seed=3, msc=200, map_name=None, warm=3, **kw):
    from as_cops_and_thieves_amd import VecCopsEnv, load_preset
    from as_cops_and_thieves_amd.selfplay.actor import PolicyActor
    name = map_name or ("labyrinth" if roster == (2, 1) else "grandbyrinth")
    env = VecCopsEnv(load_preset(name, *roster), N, num_rays=R, max_step_count=msc, seed=seed, **kw)
    env.reset()
    for t in range(warm):
        env.step(env.random_actions(t))
    actor = PolicyActor.from_checkpoint(None, env, fused=True, seed=seed)
    return env, actor


def guarded(shape, dtype, fill, band=4096):
    """A contiguous tensor of ``shape`` in the middle of a buffer whose two bands hold ``fill``; returns (view, whole, band)."""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * band,), fill, dtype=dtype, device="cuda")
    return whole[band:band + n].view(*shape), whole, band


def bands_intact(whole, band, fill):
    ref = torch.full((band,), fill, dtype=whole.dtype, device="cuda")
    return same(whole[:band], ref) and same(whole[-band:], ref)


def params_of(actor):
    from as_cops_and_thieves_amd import _learn_native as ln
    g = next(iter(actor.groups.values()))
    return g, ln.act_params({n: g.policy.w(n) for n in ln.ACT_PARAM_NAMES})


# ---------------------------------------------------------------------------------------------- 1. the sampling rule, exact
def step_sampling():
    from as_cops_and_thieves_amd import _learn_native as ln
    from as_cops_and_thieves_amd.selfplay.actor import first_max_index
    for roster in ((2, 1), (3, 2)):
        for R in (64, 90):
            for N in (1, 63, 4096, 4097):
                env, actor = make(roster, N, R)
                grp, p = params_of(actor)
                G, A = grp.G, len(actor.agents)
                gen = torch.Generator(device="cuda").manual_seed(N + R)
                h = torch.randn(G, N, 128, generator=gen, device="cuda").mul(0.5).to(torch.bfloat16)
                c = torch.randn(G, N, 128, generator=gen, device="cuda").to(torch.bfloat16)
                u = torch.rand(G, N, generator=gen, device="cuda")
                keep = (torch.rand(N, generator=gen, device="cuda") < 0.8).float()
                tag = f"{roster} R={R} N={N}"
                for tile in (32, 64):
                    hh, cc = h.clone(), c.clone()
                    actions = torch.full((N, A), 9, dtype=torch.int32, device="cuda")
                    lo = torch.zeros(G, N, 4, dtype=torch.bfloat16, device="cuda")
                    lp = torch.zeros(G, N, device="cuda")
                    ln.act_step(env.raw_outputs(), grp.indices, p, hh, cc, keep, u, actions, logits_out=lo, logp_out=lp, row_tile=tile)
                    act2 = torch.zeros(G, N, dtype=torch.long, device="cuda")
                    lp2 = torch.zeros(G, N, device="cuda")
                    actions2 = torch.full((N, A), 9, dtype=torch.int32, device="cuda")
                    ln.rollout_sample(lo, u, None, act2, lp2, None, actions2, grp.indices)
                    torch.cuda.synchronize()
                    check(torch.equal(actions, actions2), f"sampled actions {tag} tile {tile}")
                    check(same(lp, lp2), f"log-probabilities bit-equal {tag} tile {tile}")
                    check(bool(torch.isfinite(lo.float()).all()) and not same(hh, h), f"finite logits, state moved {tag} tile {tile}")
                    if tile == 32:
                        first = (lo.clone(), hh.clone(), cc.clone())
                    else:
                        check(same(lo, first[0]) and same(hh, first[1]) and same(cc, first[2]), f"row tiles 32 and 64 agree bit for bit {tag}")
                # greedy
                hh, cc = h.clone(), c.clone()
                ln.act_step(env.raw_outputs(), grp.indices, p, hh, cc, keep, u, actions, greedy=True, logits_out=lo, logp_out=lp)
                torch.cuda.synchronize()
                want = first_max_index(lo.float())
                check(torch.equal(actions.long(), want.t()), f"greedy = first maximal index {tag}")
                check(same(lo, first[0]), f"greedy logits equal sampled logits {tag}")
                # one agent uniformly at random
                hh, cc = h.clone(), c.clone()
                acts_r = torch.full((N, A), 9, dtype=torch.int32, device="cuda")
                ln.act_step(env.raw_outputs(), grp.indices, p, hh, cc, keep, u, acts_r, random_mask=0b10)
                torch.cuda.synchronize()
                check(torch.equal(acts_r[:, 1], (4.0 * u[1]).to(torch.int32).clamp(max=3)), f"random agent = min(3, int(4u)) {tag}")
                check(same(hh[1], h[1]) and same(cc[1], c[1]), f"random agent's state untouched {tag}")
                check(same(hh[0], first[1][0]) and torch.equal(acts_r[:, 0], actions2[:, 0]) and torch.equal(acts_r[:, 2], actions2[:, 2]),
                      f"network agents unaffected by the random one {tag}")
                env.check_errors()
                env.close()
                print("sampling ok:", tag, flush=True)


# ---------------------------------------------------------------------------------------------- 2. state semantics, exact
def step_state():
    from as_cops_and_thieves_amd import _learn_native as ln
    for R, N in ((64, 1000), (90, 33)):
        env, actor = make((2, 1), N, R)
        grp, p = params_of(actor)
        G, A = grp.G, len(actor.agents)
        gen = torch.Generator(device="cuda").manual_seed(5)
        h0 = torch.randn(G, N, 128, generator=gen, device="cuda").mul(0.5).to(torch.bfloat16)
        c0 = torch.randn(G, N, 128, generator=gen, device="cuda").to(torch.bfloat16)
        u = torch.rand(G, N, generator=gen, device="cuda")
        fresh = torch.rand(N, generator=gen, device="cuda") < 0.5
        NAN16 = float("nan")

        def run(h_init, c_init, keep):
            (h, hw, b), (c, cw, _) = guarded((G, N, 128), torch.bfloat16, NAN16), guarded((G, N, 128), torch.bfloat16, NAN16)
            (lo, low, _), (lp, lpw, _) = guarded((G, N, 4), torch.bfloat16, NAN16), guarded((G, N), torch.float32, NAN16)
            acts, aw, _ = guarded((N, A), torch.int32, 77)
            acts.fill_(9)
            h.copy_(h_init); c.copy_(c_init)
            ptrs = (h.data_ptr(), c.data_ptr())
            ln.act_step(env.raw_outputs(), grp.indices, p, h, c, keep, u, acts, logits_out=lo, logp_out=lp)
            torch.cuda.synchronize()
            check(ptrs == (h.data_ptr(), c.data_ptr()) and not same(h, h_init) and not same(c, c_init), f"h / c updated in place R={R}")
            for w, fill, name in ((hw, NAN16, "h"), (cw, NAN16, "c"), (low, NAN16, "logits"), (lpw, NAN16, "logp"), (aw, 77, "actions")):
                check(bands_intact(w, b, fill), f"guard bands of {name} intact R={R} N={N}")
            check(bool(((acts >= 0) & (acts <= 3)).all()) and bool(torch.isfinite(lp).all()), f"every row written R={R}")
            return lo.clone(), h.clone(), c.clone(), acts.clone(), lp.clone()

        a = run(h0, c0, (~fresh).float())
        hz, cz = h0.clone(), c0.clone()
        hz[:, fresh] = 0
        cz[:, fresh] = 0
        b_ = run(hz, cz, torch.ones(N, device="cuda"))
        check(all(same(x, y) for x, y in zip(a, b_)), f"keep = 0 equals a zeroed state with keep = 1 R={R}")
        c_ = run(hz, cz, None)
        check(all(same(x, y) for x, y in zip(b_, c_)), f"keep NULL equals keep = 1 R={R}")
        again = run(h0, c0, (~fresh).float())
        check(all(same(x, y) for x, y in zip(a, again)), f"two runs from equal inputs are bit-identical R={R}")
        env.close()
        print("state ok: R", R, flush=True)


# ---------------------------------------------------------------------------------------------- 3. accuracy against fp64
def reference_tick(P, x, h, c, keep, R):
    """fp64 on the host, no intermediate rounding.  P: name -> [G, ...] float64; x [G, N, 2R]; h, c [G, N, 128]; keep [N]."""
    F = torch.nn.functional
    G, N = x.shape[:2]
    zs, hs, cs = [], [], []
    for g in range(G):
        w = lambda n: P[n][g]
        y = torch.relu(F.conv1d(x[g].view(N, 2, R), w("features_extractor.0.weight"), w("features_extractor.0.bias"), stride=2))
        y = torch.relu(F.conv1d(y, w("features_extractor.2.weight"), w("features_extractor.2.bias"), stride=3))
        f = torch.tanh(y.reshape(N, -1) @ w("features_extractor.5.weight").t() + w("features_extractor.5.bias"))
        hp, cp = h[g] * keep.view(N, 1), c[g] * keep.view(N, 1)
        pre = f @ w("lstm.weight_ih_l0").t() + w("lstm.bias_ih_l0") + hp @ w("lstm.weight_hh_l0").t() + w("lstm.bias_hh_l0")
        i, f_, gg, o = pre.chunk(4, dim=-1)
        cn = torch.sigmoid(f_) * cp + torch.sigmoid(i) * torch.tanh(gg)
        hn = torch.sigmoid(o) * torch.tanh(cn)
        y = torch.relu(hn @ w("policy_head.0.weight").t() + w("policy_head.0.bias"))
        y = torch.relu(y @ w("policy_head.2.weight").t() + w("policy_head.2.bias"))
        zs.append(y @ w("policy_head.4.weight").t() + w("policy_head.4.bias")); hs.append(hn); cs.append(cn)
    return torch.stack(zs), torch.stack(hs), torch.stack(cs)


class Err:
    def __init__(self):
        self.mx, self.sq, self.n = 0.0, 0.0, 0

    def add(self, got, ref):
        d = (got.double().cpu() - ref).abs()
        self.mx, self.sq, self.n = max(self.mx, float(d.max())), self.sq + float((d * d).sum()), self.n + d.numel()

    @property
    def rms(self):
        return (self.sq / max(self.n, 1)) ** 0.5


def step_accuracy():
    from as_cops_and_thieves_amd import _learn_native as ln, packing
    figures = {}
    for R, scale in ((64, 1.0), (64, 4.0), (90, 4.0)):
        N, T = 4096, 16
        env, actor = make((2, 1), N, R, msc=40, warm=30)
        grp, _ = params_of(actor)
        grp.fp.lp.mul_(scale)                                    # initial weights x 4: the gates leave their linear range
        _, p = params_of(actor)
        G, A = grp.G, len(actor.agents)
        P = {n: grp.policy.w(n).detach().double().cpu() for n in ln.ACT_PARAM_NAMES}
        hk = torch.zeros(G, N, 128, dtype=torch.bfloat16, device="cuda"); ck = hk.clone()
        state_c = grp.policy.initial_state(N)
        h64 = torch.zeros(G, N, 128, dtype=torch.float64); c64 = h64.clone()
        keep = torch.zeros(N, device="cuda")
        lo = torch.zeros(G, N, 4, dtype=torch.bfloat16, device="cuda")
        acts = torch.zeros(N, A, dtype=torch.int32, device="cuda")
        errs = {k: Err() for k in ("fused logits", "fused h", "fused c", "chain logits", "chain h", "chain c")}
        tv = {"fused": 0.0, "chain": 0.0}
        for t in range(T):
            obs = env.observations()
            pin = torch.stack([packing.pack_policy_input(obs[a]) for a in grp.agents])
            x64 = pin.to(torch.bfloat16).double().cpu()
            u = torch.rand(G, N, device="cuda")
            ln.act_step(env.raw_outputs(), grp.indices, p, hk, ck, keep, u, acts, logits_out=lo)
            zc, state_c = grp.policy.forward(pin.unsqueeze(1), state_c, keep.view(1, N))
            zr, h64, c64 = reference_tick(P, x64, h64, c64, keep.double().cpu(), R)
            errs["fused logits"].add(lo, zr); errs["fused h"].add(hk, h64); errs["fused c"].add(ck, c64)
            errs["chain logits"].add(zc[:, 0], zr); errs["chain h"].add(state_c[0][0], h64); errs["chain c"].add(state_c[1][0], c64)
            pr = torch.softmax(zr, dim=-1)
            tv["fused"] += float(0.5 * (torch.softmax(lo.double().cpu(), -1) - pr).abs().sum(-1).mean()) / T
            tv["chain"] += float(0.5 * (torch.softmax(zc[:, 0].double().cpu(), -1) - pr).abs().sum(-1).mean()) / T
            raw = env.step_raw(env.random_actions(100 + t))
            keep = 1.0 - raw["terminated"].float()
        key = f"R={R} weights x{scale:g}"
        figures[key] = {}
        for q in ("logits", "h", "c"):
            for kind in ("mx", "rms"):
                a, b = getattr(errs[f"fused {q}"], kind), getattr(errs[f"chain {q}"], kind)
                figures[key][f"{q} {'max' if kind == 'mx' else 'rms'}"] = (a, b)
        figures[key]["mean TV"] = (tv["fused"], tv["chain"])
        for name, (a, b) in figures[key].items():
            print(f"accuracy {key}: {name:12s} fused {a:.6e}  chain {b:.6e}  ratio {a / b if b else float('inf'):.3f}", flush=True)
        for name, (a, b) in figures[key].items():
            check(a <= 2.0 * b, f"{key}: {name} fused {a:.4e} <= 2 x chain {b:.4e}")
        env.check_errors()
        env.close()


# ---------------------------------------------------------------------------------------------- 4. graph capture
def step_graph():
    N, T = 1024, 32
    env, actor = make((2, 1), N, 64, msc=25, warm=0)
    raw = env.raw_outputs()
    starts = torch.ones(N, dtype=torch.bool, device="cuda")
    played = torch.zeros(T, N, len(actor.agents), dtype=torch.int32, device="cuda")

    def ticks():
        for t in range(T):
            played[t].copy_(actor.act(env, starts))
            out = env.step_raw(actor.actions)
            torch.ne(out["terminated"], 0, out=starts)

    def snapshot():
        return (env.get_env_state(), {k: raw[k].clone() for k in ("obs_distance", "obs_type")}, actor.get_state(), torch.cuda.get_rng_state(),
                starts.clone())

    def restore(s):
        env.set_env_state(**s[0])
        for k, v in s[1].items():
            raw[k].copy_(v)
        actor.set_state(s[2])
        torch.cuda.set_rng_state(s[3])
        starts.copy_(s[4])

    def result():
        torch.cuda.synchronize()
        h, c = next(iter(actor.state.values()))
        return played.clone(), h.clone(), c.clone(), {k: v.clone() for k, v in env.get_env_state().items()}

    actor.reset()
    ticks()                                                      # the eager pass: every op of the tick has run once
    snap = snapshot()
    ticks()
    eager = result()
    restore(snap)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ticks()
    restore(snap)
    played.zero_()
    graph.replay()
    replayed = result()
    check(torch.equal(eager[0], replayed[0]), "graph replay: actions of all 32 ticks")
    check(same(eager[1], replayed[1]) and same(eager[2], replayed[2]), "graph replay: h and c")
    for k in eager[3]:
        check(torch.equal(eager[3][k], replayed[3][k]), f"graph replay: env state {k}")
    check(len({int(v) for v in eager[0].unique()}) == 4, "all four actions occur")
    env.check_errors()
    env.close()


# ---------------------------------------------------------------------------------------------- 5. end to end
def step_end_to_end():
    from as_cops_and_thieves_amd.selfplay.self_play import evaluate_agents_tracked
    from as_cops_and_thieves_amd.selfplay.watch import watch
    with tempfile.TemporaryDirectory() as tmp:
        sets = {}
        for name, kw in (("default", {}), ("fused", {"fused_act": True})):
            out = Path(tmp) / name
            res = watch("squarinth", 4, out, ticks=12, seed=2, log=lambda *a: None, **kw)
            files = sorted(str(f.relative_to(out)) for f in out.rglob("*") if f.is_file())
            want = sorted(["episode.json"] + [f"env_{s['env']}/frame_{t:05d}.png" for s in res["slots"] for t in range(s["frames"])])
            check(files == want, f"watch {name}: the file set follows episode.json")
            ep = json.loads((out / "episode.json").read_text())
            check(ep["envs"] == 4 and len(ep["slots"]) == 4 and all(1 <= s["length"] <= 12 for s in ep["slots"]), f"watch {name}: episode.json")
            sets[name] = {f.split("/")[0] for f in files}
        check(sets["default"] == sets["fused"], "watch: the same directories either way")
    # an actor over a trainer's own parameter buffer (FlatParams.lp: its stride and alignment) acts like one loaded from its checkpoint
    from as_cops_and_thieves_amd.selfplay.actor import PolicyActor
    from as_cops_and_thieves_amd.selfplay.mappo import CFG_AGENT, MAPPOTrainer, TrainerConfig
    env, loaded = make((2, 1), 300, 64, msc=60, warm=2, map_name="squarinth")
    runner = MAPPOTrainer(env, {"cop": CFG_AGENT, "thief": CFG_AGENT}, TrainerConfig(horizon=16, graph_rollout=False, graph_update=False), seed=8)
    shared = PolicyActor.from_trainer(runner, fused=True)
    loaded.load(runner.state_dict())
    acts = []
    for a in (shared, loaded):
        torch.manual_seed(21)
        a.reset()
        for _ in range(3):
            a.act(env)
        torch.cuda.synchronize()
        acts.append((a.actions.clone(),) + tuple(t.clone() for t in next(iter(a.state.values()))))
    check(shared.fused and all(same(x, y) for x, y in zip(*acts)), "from_trainer(fused=True) equals the actor loaded from the trainer's checkpoint")
    env.close()
    N = 512
    env, actor = make((2, 1), N, 64, msc=60, warm=0, map_name="squarinth", track_episodes=True)
    torch.manual_seed(11)
    res = []
    for k in range(4):
        if k == 2:
            snap = (env.get_env_state(), torch.get_rng_state(), torch.cuda.get_rng_state(), actor.get_state())
        if k == 3:
            env.set_env_state(**snap[0]); torch.set_rng_state(snap[1]); torch.cuda.set_rng_state(snap[2]); actor.set_state(snap[3])
        r = evaluate_agents_tracked(env, None, N, actor=actor)
        env.check_errors()
        torch.cuda.synchronize()
        h, c = next(iter(actor.state.values()))
        res.append((r, h.clone(), c.clone(), {k_: v.clone() for k_, v in env.get_env_state().items()}, torch.cuda.get_rng_state()))
        print("tracked evaluation", k, r, flush=True)
        check(abs(sum(r) - 1.0) < 1e-9, f"evaluation {k}: every episode has a winner")
    a, b = res[2], res[3]
    check(a[0] == b[0] and same(a[1], b[1]) and same(a[2], b[2]) and torch.equal(a[4], b[4]), "the fourth evaluation reproduces the third: result, h, c, generator")
    for k_ in a[3]:
        check(torch.equal(a[3][k_], b[3][k_]), f"the fourth evaluation reproduces the third: env state {k_}")
    check(bool(a[1].float().abs().sum() > 0), "the rewind left a non-trivial actor state")
    env.close()


STEPS = {"sampling": step_sampling, "state": step_state, "accuracy": step_accuracy, "graph": step_graph, "end_to_end": step_end_to_end}

if __name__ == "__main__":
    torch.set_grad_enabled(False)
    STEPS[sys.argv[1]]()
    torch.cuda.synchronize()
    print("FAILED CHECKS:" if FAILED else "ALL CHECKS PASSED", *FAILED, sep="\n  ", flush=True)
    sys.exit(1 if FAILED else 0)
