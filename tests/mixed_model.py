"""TEST INFRASTRUCTURE — the host model of a handle under pom_batch_step_mixed (include/pom_batch.h PomMixedStepSpec): RangeModel
(tests/range_model.py) extended with the SimpleAgent memory of every agent, int32 [n, 4, 16] as policy_memory() reports it, and the six
steps of the header: restart at the start (all four agents' memory zero), finished envs skipped, the mask's live agents asked
(Oracle.simple_policy at (seed, env_offset + e, tick), memory moved on), the others' moves taken from `moves`, the tick with its
bookkeeping, and the restart at the end.  Nothing of the kernel is restated.

The hooks (_wipe, _kept, _draw_env, _draw_tick, _select) are there for the deliberately wrong variants of
tests/test_mixed_model_host.py."""
import numpy as np

from tests.range_model import RangeModel, RESET_AT_START, RESET_AT_END

IDLE = 0


class MixedModel(RangeModel):
    def __init__(self, oracle, start, **options):
        super().__init__(oracle, start, **options)
        self.mems = np.zeros((self.n, 4, 16), dtype=np.int32)
        self.handle_tick = 0   # what pom_batch_set_tick / the policy calls left: a mixed step neither reads nor advances it

    # ---- where a kernel could go wrong (the wrong variants override these) ----------------------------------------------------
    def _wipe(self, e):
        self.mems[e] = 0

    def _kept(self, mask):
        """the agents whose memory a call may move: the mask's"""
        return mask

    def _draw_env(self, e, first):
        return self.env_offset + e

    def _draw_tick(self, tick):
        return tick

    def _select(self, e, a, in_mask, dead, policy_move, callers_move):
        """the move of agent a of env e: the policy's for the mask (IDLE for a dead agent of it), the caller's otherwise"""
        return (IDLE if dead else policy_move) if in_mask else callers_move

    # ---- one call -------------------------------------------------------------------------------------------------------------
    def _restart(self, e, first, log):
        super()._restart(e, first, log)
        self._wipe(e)

    def _moves_of(self, e, first, moves, mask, seed, tick):
        if mask == 0:
            return np.array(moves[e], dtype=np.int32)
        asked = self.mems[e:e + 1].copy()   # act() runs on a copy: only the memory of agents that were really asked is kept
        pol = self.oracle.simple_policy(self.states[e:e + 1], asked, seed, self._draw_env(e, first), self._draw_tick(tick))[0]
        dead = self.states["agents"]["dead"][e]
        out = np.zeros(4, dtype=np.int32)
        for a in range(4):
            in_mask = bool(mask >> a & 1)
            out[a] = self._select(e, a, in_mask, bool(dead[a]), pol[a], moves[e][a] if moves is not None else IDLE)
            if self._kept(mask) >> a & 1 and not dead[a]:
                self.mems[e, a] = asked[0, a]
        return out

    def tick_mixed(self, first, count, moves, mask, seed, tick):
        """one pom_batch_step_mixed: `moves` int32 [n, 4] indexed by the env's number in the batch (None with mask 15)"""
        assert 0 <= first and count >= 0 and first + count <= self.n and 0 <= mask <= 15 and (moves is not None or mask == 15)
        outside = np.ones(self.n, bool)
        outside[first:first + count] = False
        log = dict(first=first, count=count, restarted=[], ticked=0, by_deaths=0, marked_outside=int((self.finished[outside] != 0).sum()),
                   skipped=0, dead_in_mask=0, ub=0, mask=mask)
        self._before_call(first, count)
        for e in range(first, first + count):
            if self.done[e]:
                if self.auto_reset != RESET_AT_START:
                    log["skipped"] += 1
                    continue
                self._restart(e, first, log)
            self.finished[e] = 0
            log["dead_in_mask"] += int(any(self.states["agents"]["dead"][e][a] and mask >> a & 1 for a in range(4)))
            mv = self._moves_of(e, first, moves, mask, seed, tick)
            st = dict(done=0, winner=-1, draw=0)
            ub = self.oracle.env_step(self.states[e:e + 1], mv, st)
            self.states["agents"]["pad"][e] = 0
            self.counters[0] += 1
            self.counters[3] += ub != 0
            log["ub"] += ub != 0
            self.ubflags[e] |= ub
            self.timeout[e] = self.max_steps > 0 and int(self.states["timeStep"][e]) >= self.max_steps
            self.done[e], self.winner[e], self.draw[e] = st["done"] or self.timeout[e], st["winner"], st["draw"]
            log["ticked"] += 1
            if self.done[e]:
                self.counters[1] += 1
                log["by_deaths"] += st["done"]
                if self.auto_reset == RESET_AT_END:
                    self.terminal[e] = self.states[e]
                    self.last["winner"][e], self.last["draw"][e] = self.winner[e], self.draw[e]
                    self.last["length"][e], self.last["alive"][e] = self.states["timeStep"][e], self.states["aliveAgents"][e]
                    self._restart(e, first, log)
                    self.finished[e] = 1
        self.calls.append(log)
        return log

    def simple_ticks(self, seed, ticks):
        """pom_batch_step_simple(seed, ticks) from the handle's tick on: all four agents, the whole batch; the tick advances"""
        for _ in range(ticks):
            self.tick_mixed(0, self.n, None, 15, seed, self.handle_tick)
            self.handle_tick += 1

    # ---- everything the API can read, the agents' memory included ------------------------------------------------------------------
    def readable(self):
        return dict(super().readable(), memory=self.mems)

    def read_handle(self, env):
        return dict(super().read_handle(env), memory=env.policy_memory())
