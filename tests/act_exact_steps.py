"""The GPU steps of tests/test_gpu_act_exact.py, one per process: ``python -m tests.act_exact_steps STEP``.  Every step drives the fused
act tick (csrc/cat_act.hip) on the saturating data of tests/act_exact.py, whose right answer is known exactly, from synthesised
observation buffers (no env).  A step prints its figures and exits 0 when every check holds, 1 with the failed checks listed."""
from __future__ import annotations

import sys

import torch

from tests import act_exact as ax
from tests.act_steps import FAILED, bands_intact, check, guarded, same

NAN = float("nan")
FILL = 9                                          # the action matrix before a tick
_DATA = {}


def case_data(c):
    """Parameters, inputs and the reference of a case, computed once per data set (the row tile does not enter them)."""
    if c.seed not in _DATA:
        P, d = ax.make_params(c.sets, c.R, c.seed), ax.make_inputs(c)
        _DATA[c.seed] = (P, d, ax.reference(c, P, d), ax.reference(c, P, d, keep_one=True) if c.form == "plain" else None)
    return _DATA[c.seed]


def report(tag, name, got, want):
    """act_equal, and where it fails the mismatches: how many, and the first few with both values."""
    ok = ax.act_equal(got, want)
    if not ok:
        g = got.detach().cpu().double()
        bad = torch.where(want == 0, g.abs() > ax.ZERO_TOL, g.to(torch.bfloat16).view(torch.int16) != want.to(torch.bfloat16).view(torch.int16))
        idx = bad.nonzero()
        print(f"  {tag} {name}: {int(bad.sum())} of {bad.numel()} elements differ; first:",
              [(tuple(i.tolist()), float(g[tuple(i)]), float(want[tuple(i)])) for i in idx[:6]], flush=True)
    check(ok, f"{tag}: {name} equals the reference (bit for bit away from 0, within 2^-24 at 0)")


class Buffers:
    """The kernel's state and outputs between guard bands, and the parameter buffer of the case on the device."""

    def __init__(self, c, P, d):
        self.c = c
        (self.h, self.hw, self.band), (self.cc, self.cw, _) = guarded((c.G, c.N, ax.HID), torch.bfloat16, NAN), guarded((c.G, c.N, ax.HID), torch.bfloat16, NAN)
        self.lo, self.low, _ = guarded((c.G, c.N, 4), torch.bfloat16, NAN)
        self.acts, self.aw, _ = guarded((c.N, c.A), torch.int32, 77)
        self.h.copy_(d["h0"])
        self.cc.copy_(d["c0"])
        self.flat0 = ax.flat_params(P, c.R)
        self.flat = self.flat0.cuda()
        from as_cops_and_thieves_amd import _learn_native as ln
        self.params = ln.act_params(ax.param_views(self.flat, c.R))

    def raw(self, d, t):
        return {k: d[k][t].cuda().contiguous() for k in ("obs_distance", "obs_type", "shared_distance", "shared_type")}

    def check_guards(self, tag):
        for w, fill, name in ((self.hw, NAN, "h"), (self.cw, NAN, "c"), (self.low, NAN, "logits"), (self.aw, 77, "actions")):
            check(bands_intact(w, self.band, fill), f"{tag}: guard bands of {name} intact")
        check(same(self.flat.cpu(), self.flat0), f"{tag}: the parameter buffer and its guard bands are untouched")


def print_zero_shares(tag, ref):
    net = torch.stack([t["net"] for t in ref])
    shares = {k: ax.zero_share(torch.stack([t[k] for t in ref])[net]) for k in ("logits", "h", "c")}
    print(f"{tag}: share of elements with want = 0:", ", ".join(f"{k} {v:.4f}" for k, v in shares.items()), flush=True)


# ---------------------------------------------------------------------------------------------- 1. cat_act_step
def step_plain():
    from as_cops_and_thieves_amd import _learn_native as ln
    for c in ax.plain_cases():
        P, d, ref, ref_one = case_data(c)
        for keep_none, want in ((False, ref), (True, ref_one)):
            tag0 = c.id + (" keep=None" if keep_none else "")
            b = Buffers(c, P, d)
            for t in range(c.T):
                tag = f"{tag0} tick {t}"
                b.acts.fill_(FILL)
                b.lo.fill_(NAN)
                ptrs = (b.h.data_ptr(), b.cc.data_ptr())
                ln.act_step(b.raw(d, t), list(c.agents), b.params, b.h, b.cc, None if keep_none else d["keep"][t].cuda(), d["uniform"][t].cuda(), b.acts,
                            distance_scale=ax.DISTANCE_SCALE, type_scale=ax.TYPE_SCALE, greedy=True, logits_out=b.lo, row_tile=c.row_tile)
                torch.cuda.synchronize()
                check(ptrs == (b.h.data_ptr(), b.cc.data_ptr()), f"{tag}: h and c updated in place")
                report(tag, "logits", b.lo, want[t]["logits"])
                report(tag, "h", b.h, want[t]["h"])
                report(tag, "c", b.cc, want[t]["c"])
                acts = b.acts.cpu()
                check(torch.equal(acts[:, list(c.agents)].long(), ax.first_max(want[t]["logits"]).t()), f"{tag}: actions = first maximal index of the reference logits")
                check(bool((acts[:, 1] == FILL).all()), f"{tag}: the action column of the agent nobody plays keeps its fill")
                b.check_guards(tag)
            if not keep_none:
                print_zero_shares(c.id, want)
        print("plain ok:" if not FAILED else "plain done:", c.id, flush=True)


# ---------------------------------------------------------------------------------------------- 2. cat_act_league_step
def step_league():
    from as_cops_and_thieves_amd import _learn_native as ln
    SENT = 7.0                                                   # logits_out rows of a random segment: untouched
    for c in ax.league_cases():
        P, d, ref, _ = case_data(c)
        b = Buffers(c, P, d)
        h_first, c_first = b.h.clone(), b.cc.clone()
        for t in range(c.T):
            tag = f"{c.id} tick {t}"
            b.acts.fill_(FILL)
            b.lo.fill_(SENT)
            u = d["uniform"][t]
            ln.act_league_step(b.raw(d, t), list(c.agents), b.params, c.sets, list(ax.SEG_START), [list(r) for r in ax.SEG_SET], b.h, b.cc, d["keep"][t].cuda(),
                               u.cuda(), b.acts, distance_scale=ax.DISTANCE_SCALE, type_scale=ax.TYPE_SCALE, greedy=True, logits_out=b.lo, row_tile=c.row_tile)
            torch.cuda.synchronize()
            net = ref[t]["net"]
            report(tag, "logits (every row against its own set)", b.lo, torch.where(net.unsqueeze(-1), ref[t]["logits"], torch.full_like(ref[t]["logits"], SENT)))
            report(tag, "h", b.h, ref[t]["h"])
            report(tag, "c", b.cc, ref[t]["c"])
            acts = b.acts.cpu()[:, list(c.agents)].t().long()
            check(torch.equal(acts[net], ax.first_max(ref[t]["logits"])[net]), f"{tag}: network rows play the first maximal index of the reference logits")
            check(torch.equal(acts[~net], ax.random_action(u)[~net].long()), f"{tag}: rows of the random segments get min(3, int(4u))")
            check(bool((b.acts.cpu()[:, 1] == FILL).all()), f"{tag}: the action column of the agent nobody plays keeps its fill")
            rnd = (~net).cuda()
            check(same(b.h[rnd], h_first[rnd]) and same(b.cc[rnd], c_first[rnd]) and int(rnd.sum()) > 0, f"{tag}: h and c of the random segments bitwise untouched")
            b.check_guards(tag)
        print_zero_shares(c.id, ref)
        print("league ok:" if not FAILED else "league done:", c.id, flush=True)


# ---------------------------------------------------------------------------------------------- 3. cat_act_collect_step
def step_collect():
    """cat_act_collect_step has no greedy mode: it samples.  Which action it samples from the known ``uniform`` values is
    deliberately not pinned here (the sampling step of tests/act_steps.py does that); the step checks that act_out is the action
    matrix's column and lies in 0 .. 3, and that every log-probability is written and finite."""
    from as_cops_and_thieves_amd import _learn_native as ln
    for c in ax.collect_cases():
        P, d, ref, _ = case_data(c)
        b = Buffers(c, P, d)
        (pin, pw, band), (vin, vw, _) = guarded((c.G, c.N, 2 * c.R), torch.bfloat16, NAN), guarded((c.G, c.N, 4 * c.R), torch.bfloat16, NAN)
        (h0, h0w, _), (c0, c0w, _) = guarded((c.G, c.N, ax.HID), torch.bfloat16, NAN), guarded((c.G, c.N, ax.HID), torch.bfloat16, NAN)
        (ao, aow, _), (lp, lpw, _) = guarded((c.G, c.N), torch.int64, 77), guarded((c.G, c.N), torch.float32, NAN)
        for t in range(c.T):
            tag = f"{c.id} tick {t}"
            for x in (pin, vin, h0, c0, lp, b.lo):
                x.fill_(NAN)
            ao.fill_(-1)
            b.acts.fill_(FILL)
            before = (b.h.clone(), b.cc.clone())
            ln.act_collect_step(b.raw(d, t), list(c.agents), b.params, b.h, b.cc, d["keep"][t].cuda(), d["uniform"][t].cuda(), b.acts, ax.N_COPS, c.first_agent_state,
                                pin, vin, ao, lp, h0_out=h0, c0_out=c0, distance_scale=ax.DISTANCE_SCALE, type_scale=ax.TYPE_SCALE, logits_out=b.lo,
                                row_tile=c.row_tile)
            torch.cuda.synchronize()
            report(tag, "logits", b.lo, ref[t]["logits"])
            report(tag, "h", b.h, ref[t]["h"])
            report(tag, "c", b.cc, ref[t]["c"])
            check(same(pin.cpu(), ax.policy_rows(c, d, t).to(torch.bfloat16)), f"{tag}: policy_in rows are the scaled observations bit for bit")
            check(same(vin.cpu(), ax.value_rows(c, d, t).to(torch.bfloat16)), f"{tag}: value_in rows are the scaled shared and own observations bit for bit")
            check(same(h0, before[0]) and same(c0, before[1]), f"{tag}: h0_out / c0_out hold the state before the tick")
            acts = b.acts.cpu()
            check(torch.equal(ao.cpu(), acts[:, list(c.agents)].t().long()) and bool(((ao >= 0) & (ao <= 3)).all()), f"{tag}: act_out is the action matrix's column")
            check(bool((acts[:, 1] == FILL).all()) and bool(torch.isfinite(lp).all()), f"{tag}: the unplayed action column keeps its fill; every log-probability written")
            for w, fill, name in ((pw, NAN, "policy_in"), (vw, NAN, "value_in"), (h0w, NAN, "h0_out"), (c0w, NAN, "c0_out"), (aow, 77, "act_out"), (lpw, NAN, "logp_out")):
                check(bands_intact(w, band, fill), f"{tag}: guard bands of {name} intact")
            b.check_guards(tag)
        print_zero_shares(c.id, ref)
        print("collect ok:" if not FAILED else "collect done:", c.id, flush=True)


STEPS = {"plain": step_plain, "league": step_league, "collect": step_collect}

if __name__ == "__main__":
    torch.set_grad_enabled(False)
    STEPS[sys.argv[1]]()
    torch.cuda.synchronize()
    print("FAILED CHECKS:" if FAILED else "ALL CHECKS PASSED", *FAILED, sep="\n  ", flush=True)
    sys.exit(1 if FAILED else 0)
