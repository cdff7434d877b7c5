"""Cases for the scripted chase / evade rule (as_cops_and_thieves_amd/selfplay/scripted.py, include/cat_rollout.h): builders of synthetic ray
fans and observation buffers, and answers derived BY HAND from the rule's text -- not from either implementation.

The hand cases use R = 8, where the cone of quadrant k is ray 2k alone, q(r) = 0, 1, 1, 2, 2, 3, 3, 0 for r = 0 .. 7 and lean(r) = +1 for even
r, -1 for odd r.  Every ray is EMPTY (4) at 400 unless the case says otherwise.  ACT = (2, 1, 0, 3)."""
from __future__ import annotations

import torch

from as_cops_and_thieves_amd.selfplay.scripted import ScriptedParams

WALL, COP, THIEF, MOVABLE, EMPTY = 0, 1, 2, 3, 4
CHASE, EVADE = 0, 1
DEFAULT = ScriptedParams()
ZERO = (0, 0, 0, 0)
ODD = 0.25 + 2.0 ** -24             # uint32(u * 2^24) = 4194305: bit 0 set;  0.25 itself: 4194304, bit 0 clear


def fan(R=8, hits=None, device="cpu"):
    """(distance f16 [R], type u8 [R]) of an empty fan with ``hits`` = {ray: (type, distance)} put in."""
    d = torch.full((R,), 400.0, dtype=torch.float16)
    t = torch.full((R,), EMPTY, dtype=torch.uint8)
    for r, (ty, dist) in (hits or {}).items():
        d[r], t[r] = dist, ty
    return d.to(device), t.to(device)


def case(name, script, hits, state=ZERO, u=0.5, keep=None, params=DEFAULT, action=None, new_state=None):
    return {"name": name, "script": script, "target": THIEF if script == CHASE else COP, "hits": hits, "state": state, "u": u, "keep": keep,
            "params": params, "action": action, "new_state": new_state}


HAND_CASES = [
    # ---- the worked examples
    case("chase: thief at ray 0", CHASE, {0: (THIEF, 100)}, action=2, new_state=(1, 2, 0, 30)),
    case("evade: cop at ray 0", EVADE, {0: (COP, 100)}, action=0, new_state=(1, 0, 0, 30)),
    # q(1) = 1, lean(1) = -1: order [1, 0, 2, 3]; free[1] = 8 < 12 -> k = 0
    case("chase: thief at ray 1, wall in cone 1", CHASE, {1: (THIEF, 100), 2: (WALL, 8)}, action=2, new_state=(1, 2, 1, 30)),
    # the target itself never blocks its cone: free[0] = +inf
    case("chase: thief at ray 0 closer than clear_min", CHASE, {0: (THIEF, 5)}, action=2, new_state=(1, 2, 0, 30)),
    # ---- the memory countdown: nothing in sight, ttl > 0 -> bearing mem_ray = 2 (q = 1 -> action 1), whatever the heading says
    case("memory: ttl 30 -> 29", CHASE, {}, state=(1, 0, 2, 30), action=1, new_state=(1, 1, 2, 29)),
    case("memory: ttl 1 -> 0 still follows", CHASE, {}, state=(1, 0, 2, 1), action=1, new_state=(1, 1, 2, 0)),
    # ttl = 0: no bearing; heading 0 -> kh = ACT[0] = 2, no turn at u = 0.5 -> action 0; mem_ray and ttl stay
    case("memory: ttl 0 wanders by the heading", CHASE, {}, state=(1, 0, 2, 0), action=0, new_state=(1, 0, 2, 0)),
    case("memory: evade runs from the remembered ray", EVADE, {}, state=(1, 0, 2, 7), action=3, new_state=(1, 3, 2, 6)),
    # memory_ticks = 0: the sighting steers this tick (q(2) = 1) and leaves ttl = 0
    case("memory_ticks 0: sighting", CHASE, {2: (THIEF, 50)}, params=ScriptedParams(memory_ticks=0), action=1, new_state=(1, 1, 2, 0)),
    case("memory_ticks 0: next tick wanders", CHASE, {}, state=(1, 0, 2, 0), params=ScriptedParams(memory_ticks=0), action=0, new_state=(1, 0, 2, 0)),
    # ---- keep: 1 carries the state (bearing 2 -> action 1), 0 takes it as zero: first tick, h = min(3, int(4 * 0.5)) = 2 -> kh = 0 -> action 2
    case("keep 1 carries", CHASE, {}, state=(1, 0, 2, 5), keep=1, action=1, new_state=(1, 1, 2, 4)),
    case("keep 0 resets", CHASE, {}, state=(1, 0, 2, 5), keep=0, action=2, new_state=(1, 2, 0, 0)),
    # ---- ties on distance: the lowest ray index; otherwise the nearest, whatever its index
    case("tie: rays 2 and 6 at 100 -> ray 2", CHASE, {6: (THIEF, 100), 2: (THIEF, 100)}, action=1, new_state=(1, 1, 2, 30)),
    case("nearest: ray 6 at 50 beats ray 2 at 100", CHASE, {2: (THIEF, 100), 6: (THIEF, 50)}, action=3, new_state=(1, 3, 6, 30)),
    # ---- all cones blocked: free = [5, 9, 9, 3]; chase ray 1: order [1, 0, 2, 3] -> largest 9 first at k = 1 -> action 1
    case("blocked: chase takes the earliest of the largest", CHASE, {1: (THIEF, 100), 0: (WALL, 5), 2: (WALL, 9), 4: (WALL, 9), 6: (WALL, 3)},
         action=1, new_state=(1, 1, 1, 30)),
    # evade ray 1: k0 = 3, s = -1: order [3, 2, 0, 1] -> largest 9 first at k = 2 -> action 0
    case("blocked: evade takes the earliest of the largest", EVADE, {1: (COP, 100), 0: (WALL, 5), 2: (WALL, 9), 4: (WALL, 9), 6: (WALL, 3)},
         action=0, new_state=(1, 0, 1, 30)),
    # ---- wandering, heading 2 (kh = 0).  No turn at turn_prob 0.02 and u = 0.25
    case("wander: straight on", CHASE, {}, state=(1, 2, 0, 0), u=0.25, action=2, new_state=(1, 2, 0, 0)),
    # a forced turn (u < turn_prob = 0.5): bit 0 clear -> side -1: order [3, 1, 0, 2] -> action 3; bit 0 set -> side +1: [1, 3, 0, 2] -> action 1
    case("turn: bit 0 clear", CHASE, {}, state=(1, 2, 0, 0), u=0.25, params=ScriptedParams(turn_prob=0.5), action=3, new_state=(1, 3, 0, 0)),
    case("turn: bit 0 set", CHASE, {}, state=(1, 2, 0, 0), u=ODD, params=ScriptedParams(turn_prob=0.5), action=1, new_state=(1, 1, 0, 0)),
    # a wall ahead, no turn: u = 0.5 -> bit 0 clear -> side -1: order [0, 3, 1, 2], free[0] = 5 -> k = 3 -> action 3
    case("wander: wall ahead, side -1", EVADE, {0: (WALL, 5)}, state=(1, 2, 0, 0), u=0.5, action=3, new_state=(1, 3, 0, 0)),
    case("wander: wall ahead, side +1", EVADE, {0: (WALL, 5)}, state=(1, 2, 0, 0), u=ODD, action=1, new_state=(1, 1, 0, 0)),
    # ---- a first tick (valid = 0): h = min(3, int(4u)), never a turn.  u = 2^-7 < turn_prob: h = 0 -> kh = 2 -> action 0
    case("first tick: u = 0.9 -> h = 3", CHASE, {}, u=0.9, action=3, new_state=(1, 3, 0, 0)),
    case("first tick: no turn below turn_prob", CHASE, {}, u=2.0 ** -7, action=0, new_state=(1, 0, 0, 0)),
    # the same u with valid = 1, heading 0: a turn; u * 2^24 = 2^17, bit 0 clear -> side -1: order [1, 3, 2, 0] -> action 1
    case("later tick: the same u turns", CHASE, {}, state=(1, 0, 0, 0), u=2.0 ** -7, action=1, new_state=(1, 1, 0, 0)),
]


def case_tensors(c, device="cpu"):
    """(distance [8], type [8], u [], state [4], keep or None) of a hand case."""
    d, t = fan(8, c["hits"], device)
    return (d, t, torch.tensor(c["u"], dtype=torch.float32, device=device), torch.tensor(c["state"], dtype=torch.int32, device=device),
            None if c["keep"] is None else torch.tensor(float(c["keep"]), device=device))


def random_buffers(N, A, R, seed, device="cpu"):
    """Synthetic env-core observation buffers (obs_distance f16 [N, A, R], obs_type u8 [N, A, R]): whole-number distances in [0, 400] (so
    that ties occur), walls / movables / empty rays, in about a third of the fans a few cops AND thieves (every agent then sees its target),
    and about one fan in seven with every ray closer than the default ``clear_min`` (every cone blocked)."""
    gen = torch.Generator().manual_seed(seed)
    d = torch.randint(0, 401, (N, A, R), generator=gen).float()
    t = torch.tensor([WALL, MOVABLE, EMPTY], dtype=torch.uint8)[torch.randint(0, 3, (N, A, R), generator=gen)]
    sees = torch.rand(N, A, 1, generator=gen) < 1.0 / 3.0
    spots = torch.rand(N, A, R, generator=gen) < 4.0 / R
    who = torch.randint(COP, THIEF + 1, (N, A, R), generator=gen).to(torch.uint8)
    t = torch.where(sees & spots, who, t)
    blocked = torch.rand(N, A, 1, generator=gen) < 1.0 / 7.0
    d = torch.where(blocked, torch.randint(0, 12, (N, A, R), generator=gen).float(), d)
    return d.to(torch.float16).to(device).contiguous(), t.to(device).contiguous()
