"""The quad path's agent loop (pom_step_body.h, step_middle: lane m plays agent m, one straight-line round per chain depth) and the
bomb pass's agent look-up, on crafted one-tick states against the oracle: state AND UB flags of every case.

The cases come from tables (CASES: name, start state, Move[4]):
  - move table: for each agent index, every class of destination (off the board, passage, rigid, wood, the three power-ups, a flame,
    another agent, a BOMB item with and without a queued bomb under it — as a kicker and not, with no bomb moving, another bomb
    moving, another agent kicking this tick, a freshly planted bomb inheriting a stale direction nibble — and a destination shared
    with a live or a dead agent) times what the agent's own cell shows (him, not him, him on his own bomb, PASSAGE over his own
    bomb, another item: stepping onto a BOMB item writes the old cell even when it does not show the agent, onto passage does not);
  - row table: the four agents side by side in every assignment of indices, every set of planters among them, the others walking
    along the row (chains of depth 2, 3 and 4) or idle; the same with a flame in front of the row's head (he dies in round 0, the
    rest follow in later rounds); and with 17 - 20 bombs queued, so that some planters fit and the rest overflow;
  - bomb pass: a bomb under an agent who idles on it, under a dead agent whose item still shows, under a dead agent AND a walker who
    steps onto it this tick (the dead one is skipped, the walker bounced), with a live idle agent on it (the walker collides), with a
    live agent on it who is blocked (the walker steps on: two live agents on the bomb, the lowest index decides);
  - the bounce shortcut's neighbours: a bomb planted next to the walker that moves into the cell he leaves, a follower into that cell.
A build of the tick with the look-up's dead mask or lowest-hit rule, the vote's planted-bomb or somebody-waits term, or the old-cell
write of an agent whose cell does not show him taken out fails cases here.
Consecutive cases differ in their outcome, so a tile of 16 envs (one wavefront: 64 agents) takes every arm on the same tick.

On the CPU the cases run through the four-lane host model with its rendezvous checks (tests/emul/pom_emul_quad.cpp) and the
one-lane build; on the GPU through step_device on handles of 16 envs (one full tile) and 17 (a full tile and a ragged one), raw and
in env mode."""
import itertools

import numpy as np
import pytest

import pomcpp_amd.state as S
from pomcpp_amd.state import Item, Move
from tests.test_emul import emul_bins  # noqa: F401  (the host builds of the tick)

UB_NULL_BOMB, UB_QUEUE_OVERFLOW, UB_REVERT_LOOP = 2, 4, 8
QUAD_DIVERGED = 0x40000000

DIRS = {Move.UP: (0, -1), Move.DOWN: (0, 1), Move.LEFT: (-1, 0), Move.RIGHT: (1, 0)}
OPPOSITE = {Move.UP: Move.DOWN, Move.DOWN: Move.UP, Move.LEFT: Move.RIGHT, Move.RIGHT: Move.LEFT}
HOME = [(1, 1), (9, 1), (9, 9), (1, 9)]  # where the agents a case does not use stand idle
FACING = [Move.RIGHT, Move.DOWN, Move.LEFT, Move.UP]  # agent i's move in the move table

DESTS = (["off", "passage", "rigid", "wood", "wood_flagged", "extrabomb", "incrrange", "kick", "flame", "agent", "shared_live", "shared_dead"]
         + [f"bomb_{k}_{bm}" for k in ("walker", "kicker") for bm in ("still", "other_moving", "other_kicks", "stale_plant")]
         + ["nobomb_walker", "nobomb_kicker"])
OWN = ["shows", "hidden", "own_bomb", "hidden_own_bomb", "covered"]


def _flame(s, x, y):
    k = int(s["flames_count"])
    s["flames_queue"][k] = (x, y, 3, 1)
    s["flames_count"] = k + 1
    s["board"][y, x] = Item.FLAMES + ((x + 11 * y) << 3)


def move_case(i, dest, own):
    s = S.new_states(1)
    st = s[0]
    mv = [Move.IDLE] * 4
    d = FACING[i]
    vx, vy = DIRS[d]
    px, py = (5, 5) if dest != "off" else (5 + 5 * vx, 5 + 5 * vy)
    dx, dy = px + vx, py + vy
    j, k = (i + 1) % 4, (i + 2) % 4
    for a in range(4):
        if a != i:
            S.put_agent(st, *HOME[a], a)
    S.put_agent(st, px, py, i)
    mv[i] = d
    if dest == "rigid":
        S.put_item(st, dx, dy, Item.RIGID)
    elif dest == "wood":
        S.put_item(st, dx, dy, Item.WOOD)
    elif dest == "wood_flagged":
        S.put_item(st, dx, dy, Item.WOOD + 2)
    elif dest in ("extrabomb", "incrrange", "kick"):
        S.put_item(st, dx, dy, {"extrabomb": Item.EXTRABOMB, "incrrange": Item.INCRRANGE, "kick": Item.KICK}[dest])
    elif dest == "flame":
        _flame(st, dx, dy)
    elif dest == "agent":
        S.put_item(st, *HOME[j], Item.PASSAGE)
        S.put_agent(st, dx, dy, j)
    elif dest in ("shared_live", "shared_dead"):
        S.put_item(st, *HOME[j], Item.PASSAGE)
        S.put_agent(st, dx + vx, dy + vy, j)
        mv[j] = OPPOSITE[d]
        if dest == "shared_dead":
            S.kill(st, j)
            S.put_item(st, dx + vx, dy + vy, Item.PASSAGE)
    elif dest.startswith("bomb_"):
        _, who, bm = dest.split("_", 2)
        st["agents"][i]["canKick"] = who == "kicker"
        S.plant_bomb(st, dx, dy, j, set_item=True)
        if bm == "other_moving":
            st["agents"][j]["maxBombCount"] = 2
            S.plant_bomb(st, 4, 9, j, set_item=True)
            S.set_bomb_direction(st, 1, Move.RIGHT)
        elif bm == "other_kicks":
            st["agents"][j]["maxBombCount"] = 2
            S.plant_bomb(st, 5, 1, j, set_item=True)
            S.put_item(st, *HOME[k], Item.PASSAGE)
            S.put_agent(st, 4, 1, k)
            st["agents"][k]["canKick"] = 1
            mv[k] = Move.RIGHT
        elif bm == "stale_plant":
            slot = (int(st["bombs_index"]) + int(st["bombs_count"]) + ("own_bomb" in own)) % 20
            st["bombs_queue"][slot] = Move.RIGHT << 20
            mv[k] = Move.BOMB
    elif dest.startswith("nobomb_"):
        st["agents"][i]["canKick"] = dest == "nobomb_kicker"
        S.put_item(st, dx, dy, Item.BOMB)
    if own.startswith("hidden"):
        S.put_item(st, px, py, Item.PASSAGE)
    if own.endswith("own_bomb"):
        S.plant_bomb(st, px, py, i)
    if own == "covered":  # another item shows on his cell
        S.put_item(st, px, py, Item.EXTRABOMB)
    return s, mv


ROW_PATTERNS = ("right", "left", "even_right")


def row_case(perm, planters, pattern, flame_ahead=False, queued=0):
    """agent perm[k] at (3 + k, 5); the planters plant, the others walk along the row (or idle)"""
    s = S.new_states(1)
    st = s[0]
    mv = [Move.IDLE] * 4
    if queued:  # resting bombs on the top and bottom rows, far from the agents, in a queue that wraps around
        st["bombs_index"] = 7
        st["agents"]["maxBombCount"] = 30
        for q in range(queued):
            S.plant_bomb(st, q % 10, 10 * (q // 10), q % 4, set_item=True)
    for k, a in enumerate(perm):
        S.put_agent(st, 3 + k, 5, a)
        if (planters >> a) & 1:
            mv[a] = Move.BOMB
        elif pattern == "right" or (pattern == "even_right" and a % 2 == 0):
            mv[a] = Move.RIGHT
        elif pattern == "left":
            mv[a] = Move.LEFT
    if flame_ahead:
        _flame(st, 7, 5)
    return s, mv


def pass_cases():
    out = []
    for i in range(4):  # idles on his own bomb; a dead agent whose item still shows over a bomb
        s = S.new_states(1)
        for a in range(4):
            S.put_agent(s[0], *HOME[a], a)
        S.plant_bomb(s[0], *HOME[i], i)
        out.append((f"pass_idle_on_own_bomb_a{i}", s, [Move.IDLE] * 4))
        s = S.new_states(1)
        for a in range(4):
            S.put_agent(s[0], *HOME[a], a)
        S.plant_bomb(s[0], *HOME[i], (i + 1) % 4)
        S.kill(s[0], i)
        out.append((f"pass_dead_on_bomb_a{i}", s, [FACING[a] if a == i else Move.IDLE for a in range(4)]))
    for j, k in itertools.permutations(range(4), 2):  # j stands on a bomb whose cell shows BOMB; k steps onto it: both are there
        for kmove in (Move.RIGHT, Move.IDLE):
            s = S.new_states(1)
            st = s[0]
            for a in range(4):
                if a not in (j, k):
                    S.put_agent(st, *HOME[a], a)
            S.put_agent(st, 4, 5, k)
            S.put_agent(st, 5, 5, j)
            S.plant_bomb(st, 5, 5, [a for a in range(4) if a not in (j, k)][0], set_item=True)
            mv = [Move.IDLE] * 4
            mv[k] = kmove
            out.append((f"pass_two_on_bomb_j{j}_k{k}_{'walks' if kmove else 'idle'}", s, mv))
    return out


def cooccupant_cases():
    """The bomb pass's look-up with two position bytes equal to the bomb's: j stands on a bomb at (5, 5) whose cell shows BOMB, not
    him; k walks at it from a cell that shows him or not (no bounce shortcut then).
      - j dead: k REALLY steps on, both position bytes equal the bomb's, GetAgent skips the dead one whatever the indices and k is
        bounced.  A look-up without the dead mask leaves k there whenever j < k.
      - j alive and idle: k never arrives — an idle agent's destination is his own cell, so k collides (HasDPCollision).
      - j alive and blocked: j walks at a RIGID cell, so his destination is not his cell; k waits for him, moves in round 1, sees the
        BOMB item and (somebody waits for somebody: no shortcut) steps on.  Both live agents' position bytes equal the bomb's and the
        LOWEST index decides: k < j — the walker is found and bounced; k > j — j is found, who has not moved, and k stays.  A
        look-up that takes the highest hit drops the bomb from loop A's list when k < j and leaves k there."""
    out = []
    for j, k in itertools.permutations(range(4), 2):
        for jstate in ("live", "live_blocked", "dead", "dead_walks"):
            for kown in ("hidden", "shows"):
                s = S.new_states(1)
                st = s[0]
                for a in range(4):
                    if a not in (j, k):
                        S.put_agent(st, *HOME[a], a)
                S.put_agent(st, 4, 5, k)
                S.put_agent(st, 5, 5, j)
                S.plant_bomb(st, 5, 5, [a for a in range(4) if a not in (j, k)][0], set_item=True)
                mv = [Move.IDLE] * 4
                mv[k] = Move.RIGHT
                if jstate.startswith("dead"):
                    S.kill(st, j)
                if jstate in ("dead_walks", "live_blocked"):
                    mv[j] = Move.DOWN
                if jstate == "live_blocked":
                    S.put_item(st, 5, 6, Item.RIGID)
                if kown == "hidden":
                    S.put_item(st, 4, 5, Item.PASSAGE)
                out.append((f"pass_cooccupant_j{j}_{jstate}_k{k}_{kown}", s, mv))
    return out


def shortcut_cases():
    """The two terms of `bombs_move` that only a neighbour can make visible.  i (no kicker, his cell shows him) walks from (5, 5) onto
    a resting bomb:
      - planted: another agent plants next to i's cell into a queue slot whose stale direction nibble points at that cell — the new
        bomb moves, so the literal pair (step on, bounced back by loop A) must run, not the shortcut.  The bounce then meets the
        new bomb heading for the cell i left, pushes it back onto its planter, whose "move" has no origin: the reference's chain never
        ends and the tick raises POM_UB_REVERT_LOOP.  Nothing milder shows the term: loop A runs before any bomb moves, so only a
        bomb HEADING for the vacated cell tells the pair from the shortcut, and a planted bomb always has its planter on it.  These
        are the table's only cases with a flag other than NULL_BOMB / QUEUE_OVERFLOW (FLAGGED_ON_PURPOSE);
      - follower: an agent follows i into (5, 5) — somebody waits for somebody; the bounce that takes i back takes the follower back
        too and puts his item on his cell, which tells when that cell did not show him before."""
    out = []
    for i in range(4):
        d = FACING[i]
        vx, vy = DIRS[d]
        f = (i + 2) % 4
        for kind in ("planted_behind", "planted_beside", "follower_hidden", "follower_shows"):
            s = S.new_states(1)
            st = s[0]
            mv = [Move.IDLE] * 4
            for a in range(4):
                if a not in (i, f):
                    S.put_agent(st, *HOME[a], a)
            S.put_agent(st, 5, 5, i)
            mv[i] = d
            S.plant_bomb(st, 5 + vx, 5 + vy, (i + 1) % 4, set_item=True)
            fx, fy = (5 - vx, 5 - vy) if kind != "planted_beside" else (5 + vy, 5 + vx)
            S.put_agent(st, fx, fy, f)
            if kind.startswith("planted"):
                toward = [m for m, (ax, ay) in DIRS.items() if (fx + ax, fy + ay) == (5, 5)][0]
                st["bombs_queue"][(int(st["bombs_index"]) + int(st["bombs_count"])) % 20] = toward << 20
                mv[f] = Move.BOMB
            else:
                mv[f] = d
                if kind == "follower_hidden":
                    S.put_item(st, fx, fy, Item.PASSAGE)
            out.append((f"shortcut_a{i}_{kind}", s, mv))
    return out


def FLAGGED_ON_PURPOSE(name):
    return name.startswith("shortcut_") and "_planted_" in name


def build_cases():
    cases = []
    for own in OWN:
        for i in range(4):
            for dest in DESTS:
                s, mv = move_case(i, dest, own)
                cases.append((f"move_a{i}_{dest}_{own}", s, mv))
    perms = list(itertools.permutations(range(4)))
    for perm in perms:
        for planters in range(16):
            for pattern in ROW_PATTERNS:
                cases.append((f"row_{''.join(map(str, perm))}_p{planters:x}_{pattern}",) + row_case(perm, planters, pattern))
            if not (planters >> perm[3]) & 1:  # the head of the row walks into a flame and dies in round 0
                cases.append((f"row_{''.join(map(str, perm))}_p{planters:x}_flame",) + row_case(perm, planters, "right", flame_ahead=True))
    for queued in (17, 18, 19, 20):
        for perm in (perms[0], perms[9], perms[14], perms[23]):
            for planters in range(1, 16):
                cases.append((f"full_{queued}_{''.join(map(str, perm))}_p{planters:x}",) + row_case(perm, planters, "right", queued=queued))
    cases += pass_cases() + cooccupant_cases() + shortcut_cases()
    return cases


_table = {}


def table(oracle):
    """names, start states, moves, the oracle's states after the tick and its flags: computed once, never changed"""
    if not _table:
        cases = build_cases()
        names = [c[0] for c in cases]
        start = np.concatenate([c[1] for c in cases])
        moves = np.array([c[2] for c in cases], dtype=np.int32)
        want = start.copy()
        ubs = oracle.step_batch(want, moves)
        for a in (start, want, moves, ubs):
            a.setflags(write=False)
        _table.update(names=names, start=start, moves=moves, want=want, ubs=ubs)
    return _table


def _field_diff(got, want):
    return [f for f in got.dtype.names if got[f].tobytes() != want[f].tobytes()]


def test_the_table_says_what_it_claims(oracle):
    t = table(oracle)
    names, start, want, ubs = t["names"], t["start"], t["want"], t["ubs"]
    assert len(set(names)) == len(names)
    on_purpose = np.array([FLAGGED_ON_PURPOSE(n) for n in names])
    assert not np.any(ubs[~on_purpose] & ~np.uint32(UB_NULL_BOMB | UB_QUEUE_OVERFLOW)), "the oracle raises a flag the table is not about"
    assert on_purpose.sum() == 8 and np.all(ubs[on_purpose] == UB_REVERT_LOOP)  # shortcut_cases: the planted bomb that moves
    idx = {n: k for k, n in enumerate(names)}
    for i in range(4):
        for own in OWN:
            e, r, k = (idx[f"move_a{i}_{d}_{own}"] for d in ("extrabomb", "incrrange", "kick"))
            assert want["agents"][e, i]["maxBombCount"] == start["agents"][e, i]["maxBombCount"] + 1
            assert want["agents"][r, i]["bombStrength"] == start["agents"][r, i]["bombStrength"] + 1
            assert want["agents"][k, i]["canKick"] == 1 and start["agents"][k, i]["canKick"] == 0
            assert ubs[idx[f"move_a{i}_nobomb_kicker_{own}"]] == UB_NULL_BOMB and ubs[idx[f"move_a{i}_nobomb_walker_{own}"]] == 0
            assert want["agents"][idx[f"move_a{i}_flame_{own}"], i]["dead"] == 1
            for bm in ("still", "other_moving", "other_kicks", "stale_plant"):
                b = idx[f"move_a{i}_bomb_kicker_{bm}_{own}"]
                assert S.bomb_dir(S.queue_get(want[b], "bombs", 0)) == FACING[i], names[b]
    for k, n in enumerate(names):  # a walker is bounced off a dead co-occupant's bomb, and stopped by a live co-occupant
        if n.startswith("pass_cooccupant_"):
            walker, other = int(n.split("_k")[1][0]), int(n.split("_j")[1][0])
            stays_on = "_live_blocked_" in n and walker > other  # two live agents on the bomb: the lower index, who has not moved, is found
            assert (want["agents"][k, walker]["x"], want["agents"][k, walker]["y"]) == ((5, 5) if stays_on else (4, 5)), n
            if "_dead" in n and n.endswith("_hidden"):  # the bounce put his item on the cell that did not show him
                assert want["board"][k, 5, 4] == Item.AGENT0 + walker, n
    for i in range(4):  # a cell that does not show the agent is left alone by a step onto passage and written by a step onto a BOMB item
        onto_passage, onto_bomb = idx[f"move_a{i}_passage_covered"], idx[f"move_a{i}_bomb_kicker_still_covered"]
        assert want["board"][onto_passage, 5, 5] == Item.EXTRABOMB and want["board"][onto_bomb, 5, 5] == Item.PASSAGE
        assert start["board"][onto_bomb, 5, 5] == Item.EXTRABOMB
    full = [k for k, n in enumerate(names) if n.startswith("full_")]
    fits = sum(1 for k in full if ubs[k] == 0)
    both = sum(1 for k in full if ubs[k] == UB_QUEUE_OVERFLOW and want["bombs_count"][k] > start["bombs_count"][k])
    assert fits > 0 and both > 0 and all(want["bombs_count"][k] <= 20 for k in full)
    # rows that die at their head, and rows of every depth
    assert all(want["aliveAgents"][k] == 3 for k, n in enumerate(names) if n.endswith("_flame"))
    moved = (want["agents"]["x"] != start["agents"]["x"]).sum(axis=1)
    assert {int(m) for m, n in zip(moved, names) if n.startswith("row_") and n.endswith("_right")} == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("form", ["quad", "one_lane"])
def test_host_build_of_the_tick_plays_every_case_as_the_oracle(emul_bins, oracle, form):  # noqa: F811
    t = table(oracle)
    step = emul_bins.pom_emul_quad_step if form == "quad" else emul_bins.pom_emul_step
    bad = []
    for k, name in enumerate(t["names"]):
        s = t["start"][k:k + 1].copy()
        mv = np.ascontiguousarray(t["moves"][k])
        flags = step(s.ctypes.data, mv.ctypes.data, 0, 0, None)
        assert flags != 0xFFFFFFFF, f"{name}: not representable"
        if flags != int(t["ubs"][k]) or s.tobytes() != t["want"][k:k + 1].tobytes():
            bad.append(f"{name}: flags {flags:#x} (oracle {int(t['ubs'][k]):#x}{', the lanes diverged' if flags & QUAD_DIVERGED else ''}), "
                       f"fields {_field_diff(s[0], t['want'][k])}")
    assert not bad, f"{len(bad)} of {len(t['names'])} cases differ: " + "; ".join(bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 17])
@pytest.mark.parametrize("mode", ["raw", "env"])
def test_gpu_plays_every_case_as_the_oracle(hip_lib, oracle, mode, n):
    import torch
    from pomcpp_amd.batch import MODE_ENV, MODE_RAW, BatchEnvironment
    t = table(oracle)
    names, start, moves, ubs = t["names"], t["start"], t["moves"], t["ubs"]
    want = t["want"].copy()
    if mode == "env":
        want["timeStep"] += 1  # Environment::Step's bookkeeping
    total = len(names)
    bad = []
    with BatchEnvironment(n, mode=MODE_RAW if mode == "raw" else MODE_ENV) as env:
        for lo in range(0, total, n):
            pick = np.arange(lo, lo + n) % total  # the last handle-full wraps around to the first cases
            env.make_game(np.ascontiguousarray(start[pick]))
            env.step_device(torch.from_numpy(np.ascontiguousarray(moves[pick])).to(f"cuda:{env.device}"))
            got, flags = env.get_state(), env.status()["ubflags"]
            for e, k in enumerate(pick):
                if int(flags[e]) != int(ubs[k]) or got[e].tobytes() != want[k].tobytes():
                    bad.append(f"{names[k]} (env {e} of the cases from {lo}): flags {int(flags[e]):#x} (oracle {int(ubs[k]):#x}), "
                               f"fields {_field_diff(got[e], want[k])}")
    assert not bad, f"{len(bad)} of {total} cases differ: " + "; ".join(bad[:8])
