"""pom_batch_remember_view on the GPU (include/pom_batch.h PomMemorySpec, THE RULE): every agent's fogged view merged into its memory in
one launch, byte for byte the numpy checker's (tests/view_memory_oracle.py) tick by tick on SimpleAgent games in every reset mode, for
every radius and mask of the host tests; the properties the rule promises (radius 10, a repeat, every third tick, stale state); what
must not be written is not; the batch is left exactly as it was; the attribute outputs; a captured graph; the refusals, by name."""
import ctypes as C

import numpy as np
import pytest

import pomcpp_amd as pa
from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, RESET_AT_END, RESET_AT_START, RESET_OFF, PomError, _MemorySpec, _spec, bench_policy
from tests import view_memory_oracle as VM

pytestmark = pytest.mark.gpu
RADII, MASKS = (0, 1, 4, 10), (1, 0b1010, 15)
TICKS, CAP, SEED, BSEED = 40, 30, 20261020, 11
SENTINEL = 0xEE


def _env(n, reset=RESET_AT_END):
    """SimpleAgent's games: generated boards, a fresh one per game (the episode counters move) but with RESET_OFF"""
    fresh = reset != RESET_OFF
    env = BatchEnvironment(n, mode=MODE_ENV, auto_reset=reset, max_steps=CAP, fresh_boards=fresh, board_seed=BSEED)
    if fresh:
        env.generate(BSEED)
    else:
        env.make_game(pa.make_boards(n, seed=BSEED))
    return env


def _inputs(env):
    """what the checker takes, read off the batch: (codes, agent_attrs, env_attrs, episodes) as numpy"""
    codes, agent_attrs, env_attrs = env.observe(dtype="codes")
    return codes.cpu().numpy(), agent_attrs.cpu().numpy(), env_attrs.cpu().numpy(), env.episodes()


def _pair(n, mask=15):
    """a wiped pair on the device and its twin on the host, the views and stamp rows outside the mask holding a sentinel"""
    import torch
    memory, stamp = pa.new_view_memory(n)
    want_m, want_s = VM.new_memory(n)
    for v in range(4):
        if not (mask >> v) & 1:
            memory[:, v], stamp[:, v] = SENTINEL, 0x5EED
            want_m[:, v], want_s[:, v] = SENTINEL, 0x5EED
    torch.cuda.synchronize()
    return memory, stamp, want_m, want_s


def _remember(env, memory, stamp, *a, **kw):
    """the call, on the handle's stream, and its outputs complete for torch"""
    env.remember(memory, stamp, *a, **kw)
    env.sync()


def _same(memory, stamp, want_m, want_s, what):
    got = memory.cpu().numpy()
    bad = np.argwhere(got != want_m)
    assert bad.size == 0, f"{what}: memory differs in {len(bad)} bytes, first (env, view, plane, y, x) {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want_m[tuple(bad[0])]}"
    assert np.array_equal(stamp.cpu().numpy(), want_s), f"{what}: stamps"


@pytest.mark.parametrize("n", [48, 20])
@pytest.mark.parametrize("reset", [RESET_OFF, RESET_AT_START, RESET_AT_END], ids=["off", "at_start", "at_end"])
def test_tick_by_tick_against_the_checker(hip_lib, reset, n):
    combos = [(r, m) for r in RADII for m in MASKS]
    totals = dict.fromkeys(VM.COUNTS, 0)
    with _env(n, reset) as env:
        pairs = [_pair(n, m) for _, m in combos]
        for tick in range(TICKS + 1):
            inp = _inputs(env)
            for (radius, mask), (memory, stamp, want_m, want_s) in zip(combos, pairs):
                env.remember(memory, stamp, radius, mask)
                counts = VM.remember(want_m, want_s, *inp, radius, mask)
                for k in totals:
                    totals[k] += counts[k]
            env.sync()
            for (radius, mask), (memory, stamp, want_m, want_s) in zip(combos, pairs):
                _same(memory, stamp, want_m, want_s, f"tick {tick}, radius {radius}, mask {mask:#x}")
            env.step_simple(SEED, 1)
        # radius 10: the unfogged code planes, age 0 everywhere
        memory = pairs[combos.index((10, 15))][0].cpu().numpy()
        assert np.array_equal(memory[:, :, :5], np.broadcast_to(inp[0][:, None], memory[:, :, :5].shape)) and not memory[:, :, 5].any()
    must = ("expired_bombs", "expired_flames", "cleared_seen_elsewhere", "cleared_dead") + (("wipes",) if reset != RESET_OFF else ())
    assert all(totals[k] > 0 for k in must), totals   # (the games exercise the rule: tests/test_view_memory_host.py says why they do)


def test_a_repeat_changes_nothing_and_every_third_tick_ages_by_three(hip_lib):
    n = 48
    with _env(n) as env:
        memory, stamp, want_m, want_s = _pair(n)
        for tick in range(0, TICKS + 1, 3):
            inp = _inputs(env)
            _remember(env, memory, stamp)
            VM.remember(want_m, want_s, *inp, 4)
            _same(memory, stamp, want_m, want_s, f"tick {tick}")
            _remember(env, memory, stamp)   # the same tick again: every byte as it is
            _same(memory, stamp, want_m, want_s, f"tick {tick}, repeated")
            env.step_simple(SEED, 3)
        ages = want_m[:, :, 5]
        assert set(np.unique(ages[ages != 255]).tolist()) <= set(range(0, 255, 3)) and (ages == 3).any() and (ages == 6).any()


def test_stale_state_wipes(hip_lib):
    """restore() puts envs back to timeStep 0: their views are wiped, the others age on; a stamp of -1 wipes whatever the memory holds"""
    import torch
    n = 48
    with _env(n, RESET_OFF) as env:
        memory, stamp, want_m, want_s = _pair(n)
        for _ in range(3):
            env.step_simple(SEED, 4)
            _remember(env, memory, stamp, 1)
            VM.remember(want_m, want_s, *_inputs(env), 1)
        _same(memory, stamp, want_m, want_s, "before")
        back = [3, 17, 40]
        env.restore(back)
        inp = _inputs(env)
        assert (inp[2][back, 0] == 0).all() and (inp[2][:, 0] > 0).sum() >= n - len(back) - 8
        _remember(env, memory, stamp, 1)
        counts = VM.remember(want_m, want_s, *inp, 1)
        assert counts["wipes"] == 4 * len(back)
        _same(memory, stamp, want_m, want_s, "after restore")
        got = memory.cpu().numpy()
        assert ((got[back][:, :, 5] == 255).sum(axis=(2, 3)) >= 121 - 9).all() and ((got[[0, 16]][:, :, 5] == 255).sum(axis=(2, 3)) < 121 - 9).any()
        # a stamp of -1: "no memory yet", whatever the bytes are
        memory[5:9] = 7
        stamp[5:9] = -1
        want_m[5:9], want_s[5:9] = 7, -1
        torch.cuda.synchronize()
        _remember(env, memory, stamp, 1)
        VM.remember(want_m, want_s, *inp, 1)
        _same(memory, stamp, want_m, want_s, "after the stamps of -1")
        assert ((memory[5:9, :, 5] == 255).sum(dim=(2, 3)) >= 121 - 9).all() and not (memory[5:9, :, 0] == 7).any()


def test_range_mask_guards_and_a_second_stream(hip_lib):
    """the middle tile of three and the views of mask 0b0110: every other byte of both buffers keeps its sentinel pattern, the guard
    bytes around them too; the call on a second stream is ordered by that stream alone — the buffers are filled, merged and read on it"""
    import torch
    n, first, count, mask = 48, 16, 16, 0b0110
    with _env(n) as env:
        env.step_simple(SEED, 9)
        inp = _inputs(env)
        env.sync()
        side = torch.cuda.Stream()
        pattern_m = (np.arange(n * 2904 + 128, dtype=np.int64) * 37 % 251).astype(np.uint8)
        pattern_s = (np.arange(n * 8 + 32, dtype=np.int64) * 7919 + 100000).astype(np.int32)
        host_m, host_s = torch.from_numpy(pattern_m).pin_memory(), torch.from_numpy(pattern_s).pin_memory()
        for radius in (4, 0):
            buf_m, buf_s = torch.empty(n * 2904 + 128, dtype=torch.uint8, device="cuda"), torch.empty(n * 8 + 32, dtype=torch.int32, device="cuda")
            memory, stamp = buf_m[64:64 + n * 2904].view(n, 4, 6, 11, 11), buf_s[16:16 + n * 8].view(n, 4, 2)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                buf_m.copy_(host_m, non_blocking=True)
                buf_s.copy_(host_s, non_blocking=True)
                stamp[first:first + count, 1] = -1          # view 1 has no memory yet; view 2 holds the pattern as its memory, stamped now
                stamp[first:first + count, 2, 0] = torch.from_numpy(inp[3][first:first + count].astype(np.int32)).to("cuda", non_blocking=True)
                stamp[first:first + count, 2, 1] = torch.from_numpy(inp[2][first:first + count, 0].copy()).to("cuda", non_blocking=True) - 2
                env.remember(memory, stamp, radius, mask, first, count, side)
                got_m, got_s = buf_m.cpu(), buf_s.cpu()
            side.synchronize()
            want_m, want_s = pattern_m.copy(), pattern_s.copy()
            wm, ws = want_m[64:64 + n * 2904].reshape(n, 4, 6, 11, 11), want_s[16:16 + n * 8].reshape(n, 4, 2)
            ws[first:first + count, 1] = -1
            ws[first:first + count, 2, 0], ws[first:first + count, 2, 1] = inp[3][first:first + count], inp[2][first:first + count, 0] - 2
            VM.remember(wm, ws, *inp, radius, mask, first, count)
            assert (wm[first:first + count, 2, 5] != pattern_m[64:64 + n * 2904].reshape(n, 4, 6, 11, 11)[first:first + count, 2, 5]).any()   # view 2 aged
            assert np.array_equal(got_m.numpy(), want_m), np.argwhere(got_m.numpy() != want_m)[:5]
            assert np.array_equal(got_s.numpy(), want_s)
            # (said once more, by what must not change: the guards, the other tiles, the views outside the mask)
            g = got_m.numpy()
            assert np.array_equal(g[:64], pattern_m[:64]) and np.array_equal(g[64 + n * 2904:], pattern_m[64 + n * 2904:])
            gm, pm = g[64:64 + n * 2904].reshape(n, 4, 6, 11, 11), pattern_m[64:64 + n * 2904].reshape(n, 4, 6, 11, 11)
            assert np.array_equal(gm[:first], pm[:first]) and np.array_equal(gm[first + count:], pm[first + count:])
            assert np.array_equal(gm[:, [0, 3]], pm[:, [0, 3]])


def test_the_last_partial_tile_as_a_range(hip_lib):
    n = 20
    with _env(n) as env:
        env.step_simple(SEED, 5)
        inp = _inputs(env)
        memory, stamp, want_m, want_s = _pair(n)
        _remember(env, memory, stamp, 4, None, 16)   # no count: from 16 to the batch's end
        VM.remember(want_m, want_s, *inp, 4, 15, 16, 4)
        _same(memory, stamp, want_m, want_s, "the last tile")
        assert (want_s[:16] == -1).all() and (want_s[16:, :, 1] == 5).all()
        with pytest.raises(PomError, match="pom_batch_remember_view"):
            env.remember(memory, stamp, 4, None, 0, 8)
        with pytest.raises(PomError, match="pom_batch_remember_view"):
            env.remember(memory, stamp, 4, None, 8, 8)
        env.sync()
        _same(memory, stamp, want_m, want_s, "after the refusals")


def test_the_call_leaves_no_trace(hip_lib):
    n = 48
    with _env(n) as env:
        env.step_simple(SEED, 25)

        def readable():
            st = env.status()
            return (env.get_state().tobytes(), env.get_terminal_state().tobytes(), {k: v.tobytes() for k, v in st.items()},
                    {k: v.tobytes() for k, v in env.last_results().items()}, env.counters().tolist(), env.episodes().tobytes(),
                    env.policy_memory().tobytes(), env.chain_stats())
        before = readable()
        assert before[4][1] > 0 and any(before[5])   # games have ended, episode counters have moved
        memory, stamp, _, _ = _pair(n)
        for radius, mask in ((4, 15), (0, 1), (10, 0b1010)):
            _remember(env, memory, stamp, radius, mask)
        assert readable() == before
        # and the games go on as they would have: the same states as a batch that was never asked
        env.step_simple(SEED, 5)
        with _env(n) as twin:
            twin.step_simple(SEED, 30)
            assert twin.get_state().tobytes() == env.get_state().tobytes() and np.array_equal(twin.policy_memory(), env.policy_memory())


def test_attribute_outputs_are_observe_views(hip_lib):
    import torch
    n = 20
    with _env(n) as env:
        env.step_simple(SEED, 12)
        _, viewer_attrs, env_attrs = env.observe(dtype="codes", view_radius=4)
        memory, stamp, _, _ = _pair(n)
        va = torch.full((n, 4, 12), -7, dtype=torch.int32, device="cuda")
        ea = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _remember(env, memory, stamp, 4, 1, 16, None, None, va, ea)   # the last tile only, one agent: the attributes are the range's, all four viewers'
        assert torch.equal(va[16:], viewer_attrs[16:]) and torch.equal(ea[16:], env_attrs[16:])
        assert (va[:16] == -7).all() and (ea[:16] == -7).all()
        _remember(env, memory, stamp, 4, viewer_attrs=va)
        assert torch.equal(va, viewer_attrs) and (ea[:16] == -7).all()


def test_a_graph_of_step_and_remember_replays(hip_lib):
    """step_device_range followed by the call, on one stream, captured once: three replays equal the same calls issued one by one"""
    import torch
    n = 48
    out = []
    for graph in (False, True):
        with _env(n) as env:
            env.step_simple(SEED, 20)
            memory, stamp, _, _ = _pair(n)
            moves = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
            bench_policy(None, moves, 0, n, 3)
            env.sync()
            torch.cuda.synchronize()
            main = torch.cuda.Stream()

            def issue():
                for first in (0, 16, 32):
                    env.step_device_range(first, 16, moves, main)
                    env.remember(memory, stamp, 4, None, first, 16, main)
            if graph:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=main):
                    issue()
                assert (stamp.cpu().numpy() == -1).all()   # the capture itself runs nothing
                for _ in range(3):
                    g.replay()
            else:
                for _ in range(3):
                    issue()
            torch.cuda.synchronize()
            out.append((memory.cpu().numpy().tobytes(), stamp.cpu().numpy().tobytes(), env.get_state().tobytes()))
            assert (stamp.cpu().numpy()[:, :, 1] > 0).any()
    assert out[0] == out[1]


def test_refusals_name_the_call_and_write_nothing(hip_lib):
    import torch
    n = 48
    with _env(n) as env:
        memory, stamp, want_m, want_s = _pair(n)
        va = torch.zeros((n, 4, 12), dtype=torch.int32, device="cuda")
        lib = env._lib

        def refused(h, first, count, spec, why):
            rc = lib.pom_batch_remember_view(h, first, count, C.byref(spec) if spec is not None else None, None)
            text = lib.pom_last_error().decode()
            assert rc != 0 and "pom_batch_remember_view" in text, (why, rc, text)

        def spec(radius=4, mask=15, reserved=0, m=memory.data_ptr(), s=stamp.data_ptr(), v=None, e=None):
            return _spec(_MemorySpec, radius, mask, reserved, m, s, v, e)
        refused(env._h, 0, n, None, "a null spec")
        short = spec()
        short.struct_size -= 8
        refused(env._h, 0, n, short, "a wrong struct_size")
        for why, sp in (("radius -1", spec(radius=-1)), ("radius 11", spec(radius=11)), ("mask 0", spec(mask=0)), ("mask 16", spec(mask=16)),
                        ("reserved", spec(reserved=1)), ("null memory", spec(m=None)), ("null stamp", spec(s=None)),
                        ("misaligned memory", spec(m=memory.data_ptr() + 2)), ("misaligned stamp", spec(s=stamp.data_ptr() + 4)),
                        ("misaligned viewer_attrs", spec(v=va.data_ptr() + 8)), ("misaligned env_attrs", spec(e=va.data_ptr() + 4))):
            refused(env._h, 0, n, sp, why)
        for first, count in ((8, 16), (0, 24), (16, 8), (0, n + 16), (-16, 16)):
            refused(env._h, first, count, spec(), f"the range [{first}, {first + count})")
        refused(None, 0, n, spec(), "a null handle")
        with BatchEnvironment(64, lanes_per_env=1, envs_per_wave=64) as one_lane:
            m64, s64 = pa.new_view_memory(64)
            torch.cuda.synchronize()
            refused(one_lane._h, 0, 64, spec(m=m64.data_ptr(), s=s64.data_ptr()), "a launch shape other than the quad shape")
            with pytest.raises(PomError, match="pom_batch_remember_view"):
                one_lane.remember(m64, s64)
        env.sync()
        _same(memory, stamp, want_m, want_s, "after the refusals")
        assert not va.any()
