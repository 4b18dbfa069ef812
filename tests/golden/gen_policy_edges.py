#!/usr/bin/env python3
"""Generate tests/golden/policy_edges.npz from the COMPILED, UNMODIFIED reference agent (oracle/_ref/libpomref.so:
src/agents/simple_agent.cpp + src/bboard/strategy.cpp behind oracle/ref_shim.cpp's ref_simple_* window), on the directed corpus of
tests/policy_edge_states.py.

Runs in the build container only (needs /root/reference compiled by `make -C oracle ref`).  The fixture is data — states, memories,
draws and the reference's answers — never reference source.

  act_*   one act() each: (act_state index into states, act_agent, act_mem_in, act_draw) -> (act_move, act_mem_out).  The
          reference agent is handed the memory (ref_simple_set_memory) and reseeded until the draw it is about to make is the one
          wanted (ref_simple_peek_draw; act() makes at most one draw).  Every input is asked with the draws 0..4; where the Move or
          the memory left depends on the draw all five are kept (draw % 2 and draw % 4 are both pinned), elsewhere draw 0 only.
  game_*  short games (at most CAP ticks) from start states made of the hand-made cases, in the format of policy_traces.npz:
          four reference agents, memory zeroed at the start, each draw the stream's pom_oracle_policy_draw(SEED, env, tick, agent)
          for the env slot the game occupies on the device (game i in slot i).  The slots are laid out in wavefronts of 16 envs
          so that the first tick's wavefronts have 64, 33, 16, 17, 32, 1 and 0 agents in danger (forward-flood jobs), and the
          last wavefront is partly empty.  game_fwd_jobs holds the intended counts per wavefront.

Skip rules (the reference would read out of bounds, or the device record cannot hold the state):
  - corpus states after a tick that raises NULL_BOMB, QUEUE_OVERFLOW, REVERT_LOOP, BAD_INDEX or FLAME_QUEUE_RANGE, and every
    later tick of that entry (tests/policy_edge_states.edge_corpus_states);
  - dead agents are never asked (environment.cpp:139-146);
  - no game starts from a case with agents sharing a cell (the reference's Step faults when they all plant there);
  - a game ends when at most one agent is left, after CAP ticks, or before a tick that raises one of the flags above.
Nothing else is skipped: what the reference returns on these inputs is what is pinned.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.edge_states import FATAL, UB_FLAME_QUEUE_RANGE  # noqa: E402
from tests.golden.gen_policy_traces import ref_lib  # noqa: E402
from tests.oracle_lib import Oracle  # noqa: E402
from tests.policy_edge_states import _bomb, all_inputs, hand_cases, memories  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "policy_edges.npz")
SEED, CAP = 20261016, 40
# the wavefronts of the game layout: (games with every live agent on a ticking bomb, games with one, games with none)
WAVES = ((16, 0, 0), (8, 1, 7), (4, 0, 12), (4, 1, 11), (8, 0, 8), (0, 1, 15), (0, 0, 16), (2, 1, 2))


class RefAgent:
    """a reference SimpleAgent that is handed its memory and its draw before each act()"""

    def __init__(self, lib):
        self.lib, self.tries = lib, 0

    def act(self, state, i, mem16, draw):
        lib = self.lib
        k = 0
        while True:
            a = lib.ref_simple_new(i, 7919 * (self.tries + 1) + k)
            if lib.ref_simple_peek_draw(a) == draw:
                break
            lib.ref_simple_delete(a)
            k += 1
        self.tries += 1
        m = np.ascontiguousarray(mem16, dtype=np.int32)
        lib.ref_simple_set_memory(a, m.ctypes.data)
        mv = lib.ref_simple_act(a, state.ctypes.data)
        out = np.zeros(16, dtype=np.int32)
        lib.ref_simple_memory(a, out.ctypes.data)
        lib.ref_simple_delete(a)
        assert 0 <= mv <= 5 and np.abs(out).max() < 128
        return int(mv), out


def gen_acts(ref, oracle):
    names, states, asks = all_inputs(oracle)
    mems = memories()
    cols = {k: [] for k in ("state", "agent", "mem_in", "draw", "move", "mem_out")}
    for k, i, mname in asks:
        s = states[k:k + 1]
        m_in = mems[mname]
        answers = [ref.act(s, i, m_in, d) for d in range(5)]
        same = all(a[0] == answers[0][0] and np.array_equal(a[1], answers[0][1]) for a in answers)
        for d in ([0] if same else range(5)):
            cols["state"].append(k)
            cols["agent"].append(i)
            cols["mem_in"].append(m_in)
            cols["draw"].append(d)
            cols["move"].append(answers[d][0])
            cols["mem_out"].append(answers[d][1])
    n = len(cols["state"])
    hist = np.bincount(np.array(cols["move"]), minlength=6)
    print(f"act vectors: {n} over {states.size} states ({len(asks)} inputs); moves idle/up/down/left/right/bomb {hist.tolist()}")
    return dict(states=states.view(np.uint8).reshape(-1, 1004), state_names=np.array(names),
                act_state=np.array(cols["state"], dtype=np.int32), act_agent=np.array(cols["agent"], dtype=np.int8),
                act_mem_in=np.array(cols["mem_in"], dtype=np.int8), act_draw=np.array(cols["draw"], dtype=np.int8),
                act_move=np.array(cols["move"], dtype=np.int8), act_mem_out=np.array(cols["mem_out"], dtype=np.int8))


def game_starts():
    """start states for the wavefront layout: hand-made cases without bombs and with agent fields near play's, as they are (no
    agent in danger), with a bomb under agent 0 (one), or under every live agent (all)"""
    base = []
    for c in hand_cases():
        a = c.state["agents"][0]
        if (int(c.state["bombs_count"][0]) == 0 and int(c.state["flames_count"][0]) == 0 and int(c.state["aliveAgents"][0]) > 1
                and (a["bombCount"] >= 0).all() and (a["bombCount"] <= 3).all() and (a["maxBombCount"] >= 1).all()
                and (a["maxBombCount"] <= 8).all() and not a["dead"][0]
                and len({(int(x), int(y)) for x, y in zip(a["x"], a["y"])}) == 4):
            base.append(c.state)
    full = [s for s in base if int(s["aliveAgents"][0]) == 4]
    starts, fwd, k = [], [], 0
    for n_all, n_one, n_none in WAVES:
        jobs = 0
        for kind in ["all"] * n_all + ["one"] * n_one + ["none"] * n_none:
            s = (full if kind == "all" else base)[k % len(full if kind == "all" else base)].copy()
            k += 1
            if kind == "all":  # any strength: every agent is in danger anyway
                for i in range(4):
                    _bomb(s, int(s["agents"]["x"][0, i]), int(s["agents"]["y"][0, i]), i, 2 + (k + i) % 8, 1 + (k * 3 + i) % 5)
                jobs += 4
            elif kind == "one":  # strength 0: the bomb covers its own cell only
                _bomb(s, int(s["agents"]["x"][0, 0]), int(s["agents"]["y"][0, 0]), 0, 2 + k % 8, 0)
                jobs += 1
            starts.append(s)
        fwd.append(jobs)
    return np.concatenate(starts), np.array(fwd, dtype=np.int32)


def gen_games(ref, oracle):
    start, fwd = game_starts()
    n = start.size
    length = np.zeros(n, dtype=np.int32)
    draws, moves, asked = (np.zeros((n, CAP, 4), dtype=np.int8) for _ in range(3))
    mem = np.zeros((n, CAP, 4, 16), dtype=np.int8)
    for e in range(n):
        s = start[e:e + 1].copy()
        m = np.zeros((4, 16), dtype=np.int32)
        t = 0
        while t < CAP and s["aliveAgents"][0] > 1:
            mv = np.zeros(4, dtype=np.int32)
            for i in range(4):
                if s["agents"]["dead"][0, i]:
                    continue
                d = int(oracle.lib.pom_oracle_policy_draw(SEED, e, t, i))
                mv[i], m[i] = ref.act(s, i, m[i], d)
                draws[e, t, i], moves[e, t, i], asked[e, t, i], mem[e, t, i] = d, mv[i], 1, m[i]
            if oracle.step(s.copy(), mv) & (FATAL | UB_FLAME_QUEUE_RANGE):
                asked[e, t] = 0
                break
            ref.lib.ref_step(s.ctypes.data, mv.ctypes.data)
            s["timeStep"][0] += 1
            t += 1
        length[e] = t
    print(f"games: {n}, ticks {int(length.sum())}, act() calls {int(asked.sum())}; first-tick danger per wavefront {fwd.tolist()}")
    return dict(game_start=start.view(np.uint8).reshape(n, 1004), game_length=length, game_draws=draws, game_moves=moves,
                game_asked=asked, game_memory=mem, game_seed=np.array([SEED], dtype=np.int64), game_fwd_jobs=fwd)


def main():
    lib, oracle = ref_lib(), Oracle()
    lib.ref_simple_peek_draw.restype = C.c_int
    ref = RefAgent(lib)
    out = gen_acts(ref, oracle)
    out.update(gen_games(ref, oracle))
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
