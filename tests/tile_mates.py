"""Actors and compositions for the wavefront-mates tests (tests/test_tile_mates.py) — test infrastructure.

On the device the 16 (32, 64) envs of a wavefront share one LDS tile, one instruction stream and several loops whose trip count
is the maximum over the envs (pomcpp_amd/csrc/pom_tile.h, pom_kernels.h).  An ACTOR is one env and a script (edge_states.Entry) that pushes
one of the shared resources to its limit, or is as sensitive as possible to a mate doing so:

  deep_b_rest_dN / deep_b_push_dN   a chain of N + 1 strength-1 bombs on a boustrophedon path over the inner cells, each setting off
                      the next, the first set off INSIDE loop B on tick 0 (it rests on a flame cell / it is a moving bomb pushed
                      into one): N explosion frames, rows 0 .. N - 1 of the frame stack; the queue holds 20 bombs in every variant
  deep_b_push1_dN     the same one tick later (the moving bomb has two cells to go)
  deep_top_dN / deep_top1_dN   the control: the same chains set off by the head of the queue timing out (TickBombs), tick 0 / 1
  select_cC / select1_cC   the claim-sensitive victim: resting bomb K on cell C (the cell shows BOMB), bomb J queued after K next to
                      C and moving onto it.  Two bombs claim C, so loop_b_todo has to select K; K's turn stops J.  Were the counter
                      read as 0 or 1, K would be skipped and J would move onto C.  select1: J starts two cells away, so the
                      decisive tick is tick 1.  select_idx13 / select_idx19: the queue's head wrapped; select_pairs20: ten pairs
  claims_full         20 moving bombs whose positions and targets touch all 31 dwords of the claim map
  bounce_H            AgentBombChainReversion of H hops started from loop B (a kicked bomb collides: the `unforeseen_` path)
  quiet_*             nothing happens: idle agents; all dead; one alive (ENV mode: done after a tick); late_K: timeStep = ENV_CAP - K
  edge_*              taken over from tests/edge_states.py: a > 20-flame queue, a full bomb queue, LOST_AGENT

A COMPOSITION is a batch: int actor index per env, for one launch shape.  Env e of a batch sits in wavefront e // EPW at column
e % EPW (a wavefront holds EPW / 16 consecutive 16-env HBM tiles, column = 16 * tile-in-wavefront + lane).  Families: overlay,
pairs, crowd, restart (below).  Everything here is numpy; nothing needs a GPU.
"""
from __future__ import annotations

import os
import re

import numpy as np

import pomcpp_amd.state as S
from pomcpp_amd.state import Item
from tests.edge_states import Entry, _base, _flame_cell, _idle, _script, corpus
from tests.edge_states import B, D, I, L, R, U  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICKS = 16           # every actor's script has this many ticks
DEPTHS = (1, 2, 5, 10, 15, 19)   # frames pushed by the deep_* variants; 19 = 20 queued bombs, each but the first pushes one
MAX_DEPTH = DEPTHS[-1]
DIR = {(0, -1): 1, (0, 1): 2, (-1, 0): 3, (1, 0): 4}  # Direction (bboard.hpp): UP, DOWN, LEFT, RIGHT
CORNERS = {(0, 0), (10, 0), (10, 10), (0, 10)}
ENV_CAP = 6          # the step cap of the restart family; quiet_late_K counts back from it


# ------------------------------------------------------------------------------------------------------------ the layout
def layout():
    """what the overlay family was derived from, read out of the headers"""
    k = open(os.path.join(ROOT, "pomcpp_amd", "csrc", "pom_tile.h")).read()
    b = open(os.path.join(ROOT, "pomcpp_amd", "csrc", "pom_step_body.h")).read()
    row = lambda name: re.search(name + r" = POM_REC_DWORDS \+ (\d+)", k).group(1)  # noqa: E731
    return dict(row_stack=int(row("ROW_STACK")), row_claims=int(row("ROW_CLAIMS")),
                stack_depth=int(re.search(r"#define POM_STACK_DEPTH (\d+)", b).group(1)),
                claim_stride=int(re.search(r"claim_map\(\) const \{[^}]*\* (\d+); \}", k).group(1)),
                frame=re.search(r"a\.set_frame\(sp, ([^;]*)\);", b).group(1))


LAYOUT = dict(row_stack=5, row_claims=5, stack_depth=21, claim_stride=124,
              frame="x | (y << 4) | (s << 8) | (rstar << 12) | (d << 15) | (rem << 19)")


def alias(epw, d, a):
    """frame d of the env in column a is the dword at byte (d * epw + a) * 4 of the region that also holds the claim maps,
    [env][124 bytes]: (column whose map it lies in, byte of that map)"""
    byte = (d * epw + a) * 4
    return byte // 124, byte % 124


# ------------------------------------------------------------------------------------------------------------ the actors
def snake():
    """rows 1, 3, 5, 7, 9 of the inner cells joined at alternating ends: consecutive cells adjacent, no other two are"""
    path = []
    for r, y in enumerate((1, 3, 5, 7, 9)):
        xs = list(range(1, 10)) if r % 2 == 0 else list(range(9, 0, -1))
        path += [(x, y) for x in xs]
        if y < 9:
            path.append((xs[-1], y + 1))
    return path


def _bombers(s, n=30, strength=1):
    for a in range(4):
        s["agents"][0, a]["maxBombCount"] = n
        s["agents"][0, a]["bombStrength"] = strength


def deep(trigger, depth):
    """trigger: rest, push, push1 (loop B, tick 0 / 0 / 1), top, top1 (TickBombs, tick 0 / 1)"""
    s = _base()
    _bombers(s)
    path = snake()
    chain = path[2:2 + depth + 1]              # chain[0] goes off first
    rest = path[2 + depth + 2:][:20 - len(chain)]  # one cell free, then the bombs that only fill the queue
    fx, fy = chain[0]
    if trigger in ("rest", "push", "push1"):
        s["board"][0, fy, fx] = _flame_cell(fx, fy)
        s["flames_queue"][0, 0] = (fx, fy, 3, 0)
        s["flames_count"] = 1
    k = 0
    for i, (x, y) in enumerate(chain):
        life = 10
        if i == 0 and trigger in ("top", "top1"):
            life = 1 if trigger == "top" else 2
        if i == 0 and trigger in ("push", "push1"):
            x, y = path[1] if trigger == "push" else path[0]
        on_flame = i == 0 and trigger == "rest"
        S.plant_bomb(s[0], x, y, k % 4, set_item=not on_flame, life_time=life)
        if i == 0 and trigger in ("push", "push1"):
            S.set_bomb_direction(s[0], 0, 4)
        k += 1
    for (x, y) in rest:
        S.plant_bomb(s[0], x, y, k % 4, set_item=True, life_time=10)
        k += 1
    assert int(s["bombs_count"][0]) == 20
    name = {"rest": "deep_b_rest", "push": "deep_b_push", "push1": "deep_b_push1", "top": "deep_top", "top1": "deep_top1"}[trigger]
    return Entry(f"{name}_d{depth}", s, _idle(TICKS), f"a chain of {depth + 1} bombs, {depth} frames, trigger {trigger}")


def _neighbour(x, y, dist):
    """a cell `dist` away in a straight line from which a bomb can travel to (x, y): (cell, direction)"""
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        cells = [(x + dx * k, y + dy * k) for k in range(1, dist + 1)]
        if all(0 <= cx <= 10 and 0 <= cy <= 10 and (cx, cy) not in CORNERS for cx, cy in cells):
            return cells[-1], DIR[(-dx, -dy)]
    raise AssertionError((x, y))


def select(c, phase=0, index=0):
    s = _base()
    _bombers(s)
    s["bombs_index"] = index
    x, y = c % 11, c // 11
    S.plant_bomb(s[0], x, y, 1, set_item=True)           # K
    (jx, jy), d = _neighbour(x, y, 1 + phase)
    S.plant_bomb(s[0], jx, jy, 2, set_item=True)         # J
    S.set_bomb_direction(s[0], 1, d)
    name = f"select{phase or ''}_c{c}" if index == 0 else f"select_idx{index}"
    return Entry(name, s, _idle(TICKS), f"K rests on cell {c}, J moves onto it on tick {phase}: K must be selected")


def select_pairs20():
    s = _base()
    _bombers(s)
    ks = [(5, y) for y in range(1, 6)] + [(8, y) for y in range(5, 10)]
    js = [((4, y), 4) for y in range(1, 6)] + [((9, y), 3) for y in range(5, 10)]
    order = []
    for i in range(5):  # K, J interleaved
        order += [("k", i), ("j", i)]
    order += [("k", i) for i in range(5, 10)] + [("j", i) for i in range(5, 10)]  # all Ks, then their Js
    for n, (what, i) in enumerate(order):
        (x, y) = ks[i] if what == "k" else js[i][0]
        S.plant_bomb(s[0], x, y, n % 4, set_item=True)
        if what == "j":
            S.set_bomb_direction(s[0], n, js[i][1])
    return Entry("select_pairs20", s, _idle(TICKS), "20 bombs, ten pairs contending for ten cells")


def claims_full():
    s = _base(corners=False)
    for a, (x, y) in enumerate(((0, 0), (10, 0), (5, 6), (0, 10))):
        S.put_agent(s[0], x, y, a)
    _bombers(s)
    cells = [8 * i + 3 for i in range(15) if i != 5] + [42, 44, 119]
    movers = [(c, 4) for c in cells] + [(2 * 11 + 0, 2), (5 * 11 + 2, 1), (8 * 11 + 5, 2)]
    for n, (c, d) in enumerate(movers):
        S.plant_bomb(s[0], c % 11, c // 11, n % 4, set_item=True)
        S.set_bomb_direction(s[0], n, d)
    assert int(s["bombs_count"][0]) == 20
    return Entry("claims_full", s, _idle(TICKS), "20 moving bombs: positions and targets in all 31 dwords of the claim map")


# hops: (agents in the row, moving bombs [(x, y, direction)] queued before X)
BOUNCES = {1: (1, ()), 2: (2, ()), 3: (3, ()), 4: (4, ()),
           5: (3, ((3, 5, 3),)), 6: (2, ((3, 5, 3), (4, 5, 3))), 7: (3, ((2, 5, 3), (3, 5, 3)))}


def bounce(hops):
    """agents in a row on y = 5 step right; the first kicks bomb X on (5, 5), whose target holds the resting bomb Y: X is stopped in
    loop B and the kicker bounces back into the agent behind it, and so on down the row.  For more than four hops bombs that roll
    LEFT along the row (under the agents) head for the cells the row falls back to: each is pushed back onto the agent behind it,
    which bounces a second time (found by a search over such bombs with the instrumented host build; the hop counts are asserted
    in tests/test_tile_mates.py)"""
    row, rollers = BOUNCES[hops]
    s = _base(corners=False)
    free = [(0, 0), (10, 0), (10, 10), (0, 10)]
    train = list(range(4 - row, 4))  # agent 3 is the kicker
    for a in range(4):
        if a in train:
            S.put_agent(s[0], 1 + train.index(a) + (4 - row), 5, a)
        else:
            S.put_agent(s[0], *free[a], a)
    _bombers(s)
    s["agents"][0, 3]["canKick"] = 1
    for n, (x, y, d) in enumerate(rollers):
        if int(s["board"][0, y, x]) == Item.PASSAGE:
            s["board"][0, y, x] = Item.BOMB
        S.plant_bomb(s[0], x, y, 0)
        S.set_bomb_direction(s[0], n, d)
    S.plant_bomb(s[0], 5, 5, 0, set_item=True)  # X
    S.plant_bomb(s[0], 6, 5, 1, set_item=True)  # Y
    mv = [R if a in train else I for a in range(4)]
    return Entry(f"bounce_{hops}", s, np.concatenate([_script((mv, 1)), _idle(TICKS - 1)]), f"a bounce-back chain of {hops} hops from loop B")


def quiet():
    out = []
    out.append(Entry("quiet_idle", _base(), _idle(TICKS), "an empty board, four idle agents"))
    s = _base()
    for a, (x, y) in enumerate(((0, 0), (10, 0), (10, 10), (0, 10))):
        s["board"][0, y, x] = Item.PASSAGE
    S.kill(s[0], 0, 1, 2, 3)
    out.append(Entry("quiet_all_dead", s, _idle(TICKS), "all four agents dead"))
    s = _base()
    for a, (x, y) in ((1, (10, 0)), (2, (10, 10)), (3, (0, 10))):
        s["board"][0, y, x] = Item.PASSAGE
    S.kill(s[0], 1, 2, 3)
    out.append(Entry("quiet_one_alive", s, _idle(TICKS), "one agent alive: in ENV mode done after the first tick, then not stepped"))
    for k in (1, 2, 3):
        s = _base()
        s["timeStep"] = ENV_CAP - k
        out.append(Entry(f"quiet_late_{k}", s, _idle(TICKS), f"timeStep = cap - {k}: finishes on tick {k - 1}"))
    return out


def taken_over(oracle):
    by = {e.name: e for e in corpus(oracle)}
    out = []
    for name, own_script in (("fq_issue_40_head4", True), ("fq_spawn21", True), ("fq_stuck21_rays", True),
                             ("bomb_queue_full_index19", False), ("ub_lost_agent", True)):
        e = by[name]
        mv = _idle(TICKS)
        if own_script:
            k = min(len(e.moves), TICKS)
            mv[:k] = e.moves[:k]
        out.append(Entry("edge_" + name, e.start.copy(), mv, e.prop))
    return out


SELECT_CELLS = tuple(range(3, 120, 4))  # the cells whose counter is the top byte of a dword of the claim map


def actors(oracle):
    out = []
    for trig in ("rest", "push", "push1", "top", "top1"):
        out += [deep(trig, d) for d in DEPTHS]
    for phase in (0, 1):
        out += [select(c, phase) for c in SELECT_CELLS]
    out += [select(60, 0, 13), select(60, 0, 19), select_pairs20(), claims_full()]
    out += [bounce(h) for h in sorted(BOUNCES)]
    out += quiet() + taken_over(oracle)
    names = [e.name for e in out]
    assert len(set(names)) == len(names)
    for e in out:
        e.start["agents"]["pad"] = 0
        if not e.name.startswith("edge_"):  # nobody can plant into a full queue, whatever moves a test plays (random, SimpleAgent)
            ag = e.start["agents"][0]
            own = ag["bombCount"] > 0
            ag["maxBombCount"][own] = ag["bombCount"][own]
        assert e.moves.shape == (TICKS, 4)
    return out


def kind(name):
    """the actor's kind, for the pairs family"""
    for k in ("deep_b", "deep_top", "select", "claims_full", "bounce", "quiet", "edge"):
        if name.startswith(k):
            return k
    raise AssertionError(name)


AGGRESSORS = ("deep_b", "deep_top", "claims_full", "bounce")
VICTIMS = ("select", "claims_full", "bounce", "quiet", "edge", "deep_b")


def solo_traces(oracle, entries, ticks=TICKS):
    """the oracle's run of every actor alone: states uint8[A, ticks, 1004], flags uint32[A, ticks]"""
    states = np.zeros((len(entries), ticks, 1004), dtype=np.uint8)
    ubs = np.zeros((len(entries), ticks), dtype=np.uint32)
    for i, e in enumerate(entries):
        s = e.start.copy()
        for t in range(ticks):
            ubs[i, t] = oracle.step(s, e.moves[t])
            s["agents"]["pad"] = 0
            states[i, t] = np.frombuffer(s.tobytes(), dtype=np.uint8)
    return states, ubs


# ------------------------------------------------------------------------------------------------------------ compositions
class Cast:
    """actor indices by name and kind"""

    def __init__(self, entries):
        self.names = [e.name for e in entries]
        self.ix = {n: i for i, n in enumerate(self.names)}
        self.kinds = [kind(n) for n in self.names]
        self.filler = [self.ix[n] for n in ("quiet_idle", "claims_full", "bounce_1", "quiet_all_dead", "bounce_2", "bounce_3",
                                            "quiet_one_alive", "bounce_4", "bounce_5", "claims_full", "bounce_6", "bounce_7")]

    def deep_b(self, d, phase, alt=0):
        """the deep_b variant with the fewest frames that still writes frame d, going off on tick `phase`"""
        n = min(x for x in DEPTHS if x > d)
        return self.ix[f"deep_b_push1_d{n}" if phase else (f"deep_b_push_d{n}" if alt else f"deep_b_rest_d{n}")]

    def of_kind(self, k):
        return [i for i, kk in enumerate(self.kinds) if kk == k]


def _fill(cast, waves, epw):
    """waves: list of {column: actor}; the free columns get the fillers in rotation -> int32[len(waves) * epw]"""
    out = np.zeros(len(waves) * epw, dtype=np.int32)
    r = 0
    for w, cols in enumerate(waves):
        for c in range(epw):
            if c in cols:
                out[w * epw + c] = cols[c]
            else:
                out[w * epw + c] = cast.filler[r % len(cast.filler)]
                r += 1
    return out


def overlay_pairs(epw):
    """every (d, A) of the aliasing arithmetic and where it lands: (d, A, B, cell) with the frame's top byte on the counter of
    `cell` in column B's map; pad bytes and B == A skipped"""
    out = []
    for d in range(MAX_DEPTH):
        for a in range(epw):
            b, byte = alias(epw, d, a)
            c = byte + 3
            if c > 120 or b == a:
                continue
            assert b < epw
            out.append((d, a, b, c))
    return out


def overlay(cast, epw):
    """for every pair of overlay_pairs and both phases: a wavefront with a deep_b that writes frame d in column A (going off on
    tick `phase`) and select / select1 on the aliased cell in column B.  Pairs share a wavefront where their columns agree.
    Returns (actor per env, the list of (wave, d, A, B, cell, phase))."""
    waves, placed = [], []
    for phase in (0, 1):
        first = len(waves)
        for (d, a, b, c) in overlay_pairs(epw):
            agg = cast.deep_b(d, phase, alt=(d + a) & 1)
            vic = cast.ix[f"select{phase or ''}_c{c}"]
            for w in range(first, len(waves) + 1):
                if w == len(waves):
                    waves.append({})
                cols = waves[w]
                if cols.get(a, agg) == agg and cols.get(b, vic) == vic:
                    cols[a], cols[b] = agg, vic
                    placed.append((w, d, a, b, c, phase))
                    break
    return _fill(cast, waves, epw), placed


def pairs(cast, epw):
    """every ordered (aggressor kind, victim kind) shares a wavefront, and every victim kind sits at every column with a deep_b or
    claims_full mate: wavefront (v, c) has a member of victim kind v at column c, one member of every aggressor kind in the
    columns after it, members of v's kind cycling with c"""
    waves = []
    for v in VICTIMS:
        members = cast.of_kind(v)
        for c in range(epw):
            cols = {c: members[c % len(members)]}
            for j, agg in enumerate(AGGRESSORS):
                am = cast.of_kind(agg)
                if agg == "deep_b":
                    am = [i for i in am if cast.names[i].endswith(f"_d{MAX_DEPTH}")]
                cols[(c + 1 + j) % epw] = am[(c + j) % len(am)]
            waves.append(cols)
    return _fill(cast, waves, epw)


def crowd(cast, epw, tail):
    """wavefronts with 0, 1, 2, epw - 1 and epw envs of one heavy kind (the deepest deep_b, claims_full), the rest quiet; then a last,
    ragged wavefront of `tail` envs"""
    quiet_i = cast.ix["quiet_idle"]
    out = []
    for heavy in (cast.ix[f"deep_b_rest_d{MAX_DEPTH}"], cast.ix["claims_full"], cast.ix[f"deep_top_d{MAX_DEPTH}"]):
        for k in (0, 1, 2, epw - 1, epw):
            wave = [quiet_i] * epw
            for j in range(k):
                wave[(j * 7 + 3) % epw if k <= 2 else j] = heavy
            if k == epw - 1:
                wave = wave[-1:] + wave[:-1]  # the quiet one at column 0 ... and at the last column for the other kinds
            out += wave
    mix = [cast.ix[f"deep_b_push_d{MAX_DEPTH}"], cast.ix["select_c63"], cast.ix["claims_full"], cast.ix["bounce_4"], cast.ix["select_pairs20"]]
    out += [mix[j % len(mix)] for j in range(tail)]
    return np.array(out, dtype=np.int32)


def restart(cast, epw):
    """ENV mode with the cap at ENV_CAP (every env restarts every ENV_CAP ticks at the latest): wavefronts in which 0, 1, 2, epw - 1, epw envs finish on tick 0 (quiet_late_1: timeStep =
    cap - 1) — at both ends and in the middle —, the others deep_b mates that go off on that tick (rest / push) and on the tick
    after (push1), when the finished columns are rewritten"""
    late = cast.ix["quiet_late_1"]
    mates = [cast.ix[f"deep_b_rest_d{MAX_DEPTH}"], cast.ix[f"deep_b_push1_d{MAX_DEPTH}"], cast.ix[f"deep_b_push_d{MAX_DEPTH}"],
             cast.ix["deep_b_push1_d10"], cast.ix["claims_full"]]
    out = []
    for k, where in ((0, ()), (1, (0,)), (1, (epw - 1,)), (1, (epw // 2,)), (2, (0, epw - 1)), (2, (epw // 2 - 1, epw // 2)),
                     (epw - 1, tuple(range(1, epw))), (epw - 1, tuple(range(epw - 1))), (epw, tuple(range(epw)))):
        assert len(where) == k
        out += [late if c in where else mates[(c + k) % len(mates)] for c in range(epw)]
    # the same with games that finish one and two ticks later, mixed into one wavefront
    out += [cast.ix[f"quiet_late_{1 + c % 3}"] if c % 2 else mates[c % len(mates)] for c in range(epw)]
    return np.array(out, dtype=np.int32)


def batch(entries, who, ticks=TICKS):
    """start states STATE_DTYPE[n] and moves int32[ticks, n, 4] of a composition"""
    start = np.concatenate([entries[i].start for i in who])
    moves = np.stack([entries[i].moves[:ticks] for i in who], axis=1).astype(np.int32)
    return start, np.ascontiguousarray(moves)
