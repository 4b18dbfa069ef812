"""What BatchEnvironment's calls ask of their device tensors (pomcpp_amd/batch.py _device_tensor, _out_tensor): every tensor argument of
step_device, step_device_many, step_device_range (plain, per-agent and fogged-view forms), copy_envs (tensor form), observe(out=),
forecast, move_safety, rollout, rollout_jobs, expand and move_table(others=) is
refused with a ValueError that names the argument when its element type or its shape is wrong, when it is a non-contiguous view of a
larger tensor, and when it lives on the CPU — and a refused call has done nothing: state, counters and episode numbers are what they were.

One handle of 20 envs, one whole tile and a short one; nothing is launched by a refused call, so no larger shape can fail differently."""
import numpy as np
import pytest

N, M, SAMPLES, HORIZON = 20, 7, 2, 4   # envs; jobs of the list-driven calls; rollout samples and horizon


def _handle():
    import pomcpp_amd as pa
    from pomcpp_amd.batch import BatchEnvironment, DIST_RANDOM, MODE_ENV
    env = BatchEnvironment(N, device=0, mode=MODE_ENV, max_steps=800)
    env.make_game(pa.make_boards(N, seed=5))
    env.step_random(3, DIST_RANDOM, ticks=5)   # counters that are not zero
    return env


def range_rows(env, i32, u8, good):
    """_table's rows of step_device_range, the one tensor-taking call that makes no runtime call: tests/test_wrapper_args_host.py drives
    them without a GPU.  good(shape, dtype): a right tensor for the arguments that are not the row's; the range is the first tile."""
    mv = good((N, 4), i32)
    planes, views = good((N, 16, 11, 11), u8), good((N, 4, 16, 11, 11), u8)
    step = lambda **kw: env.step_device_range(0, 16, mv, **kw)  # noqa: E731
    return [
        ("step_device_range", "moves", "moves", i32, (N, 4), False, lambda t: env.step_device_range(0, 16, t)),
        ("step_device_range", "codes", "codes", u8, (N, 5, 11, 11), False, lambda t: step(codes=t)),
        ("step_device_range", "planes", "planes", u8, (N, 16, 11, 11), False, lambda t: step(planes=t)),
        ("step_device_range(per_agent)", "planes", "planes", u8, (N, 4, 16, 11, 11), False, lambda t: step(planes=t, per_agent=True)),
        ("step_device_range", "agent_attrs", "agent_attrs", i32, (N, 4, 8), False, lambda t: step(planes=planes, agent_attrs=t)),
        ("step_device_range", "env_attrs", "env_attrs", i32, (N, 4), False, lambda t: step(planes=planes, env_attrs=t)),
        ("step_device_range(view_radius)", "codes", "codes", u8, (N, 4, 5, 11, 11), False, lambda t: step(codes=t, view_radius=4)),
        ("step_device_range(view_radius)", "planes", "planes", u8, (N, 4, 16, 11, 11), False, lambda t: step(planes=t, view_radius=4)),
        ("step_device_range(view_radius)", "viewer_attrs", "viewer_attrs", i32, (N, 4, 12), False,
         lambda t: step(planes=views, view_radius=4, viewer_attrs=t)),
        ("step_device_range(view_radius)", "env_attrs", "env_attrs", i32, (N, 4), False, lambda t: step(planes=views, view_radius=4, env_attrs=t)),
    ]


def other_rows(env, i8, i32, i64, u8, good):
    """_table's rows of every other call, with the same good(shape, dtype); tests/test_wrapper_args_host.py drives these too, torch and
    the library stood in for"""
    src = good((M,), i64).fill_(-1)   # entries without a job: even a call that went through would change nothing
    mv = good((M, 4), i32)
    return [
        ("step_device", "moves", "moves", i32, (N, 4), False, lambda t: env.step_device(t)),
        ("step_device_many", "moves", "moves", i32, (3, N, 4), True, lambda t: env.step_device_many(t)),
        ("copy_envs", "src", "src", i64, (N,), True, lambda t: env.copy_envs(t)),
        ("observe", "out", "out", u8, (N, 16, 11, 11), False, lambda t: env.observe(out=t)),
        ("forecast", "moves", "moves", i32, (N, 4), False, lambda t: env.forecast(HORIZON, moves=t)),
        ("forecast", "out[flame_tick]", "flame_tick", u8, (N, 11, 11), False, lambda t: env.forecast(HORIZON, out={"flame_tick": t})),
        ("forecast", "out[agent_tick]", "agent_tick", i32, (N, 4), False, lambda t: env.forecast(HORIZON, out={"agent_tick": t})),
        ("forecast", "out[ubflags]", "ubflags", i32, (N,), False, lambda t: env.forecast(HORIZON, out={"ubflags": t}, ubflags=True)),
        ("move_safety", "moves", "moves", i32, (N, 4), False, lambda t: env.move_safety(HORIZON, moves=t)),
        ("move_safety", "out[death_tick]", "death_tick", i8, (N, 4, 6), False, lambda t: env.move_safety(HORIZON, out={"death_tick": t})),
        ("move_safety", "out[escape_tick]", "escape_tick", i8, (N, 4, 6), False, lambda t: env.move_safety(HORIZON, out={"escape_tick": t})),
        ("rollout", "moves", "moves", i32, (N, 4), False, lambda t: env.rollout(HORIZON, SAMPLES, 1, moves=t)),
        ("rollout", "out", "out", i32, (SAMPLES, N), False, lambda t: env.rollout(HORIZON, SAMPLES, 1, out=t)),
        ("rollout(simple=)", "moves", "moves", i32, (N, 4), False, lambda t: env.rollout(HORIZON, SAMPLES, 1, moves=t, simple=[0])),
        ("rollout_jobs", "src", "src", i64, (M,), True, lambda t: env.rollout_jobs(t, HORIZON, SAMPLES, 1)),
        ("rollout_jobs", "moves", "moves", i32, (M, 4), False, lambda t: env.rollout_jobs(src, HORIZON, SAMPLES, 1, moves=t)),
        ("rollout_jobs", "out", "out", i32, (SAMPLES, M), False, lambda t: env.rollout_jobs(src, HORIZON, SAMPLES, 1, out=t)),
        ("expand", "src", "src", i64, (M,), True, lambda t: env.expand(t, mv)),
        ("expand", "moves", "moves", i32, (M, 4), False, lambda t: env.expand(src, t)),
        ("expand", "out", "out", i32, (M,), False, lambda t: env.expand(src, mv, out=t)),
        ("expand", "codes", "codes", u8, (N, 5, 11, 11), False, lambda t: env.expand(src, mv, codes=t)),
        ("expand", "planes", "planes", u8, (N, 16, 11, 11), False, lambda t: env.expand(src, mv, planes=t)),
        ("expand(per_agent)", "planes", "planes", u8, (N, 4, 16, 11, 11), False, lambda t: env.expand(src, mv, planes=t, per_agent=True)),
        ("move_table", "others", "others", i32, (N, 4), False, lambda t: env.move_table(0, HORIZON, SAMPLES, 1, others=t)),
    ]


def _table(env, torch):
    """(call, argument, the text that names it, element type, shape, free: the first dimension is the caller's, the call given a tensor)"""
    dev = torch.device("cuda", 0)
    good = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
    return range_rows(env, torch.int32, torch.uint8, good) + other_rows(env, torch.int8, torch.int32, torch.int64, torch.uint8, good)


def _bad(torch, dtype, shape, free):
    """the wrong tensors for an argument of `dtype` and `shape`: (what is wrong, tensor)"""
    dev = torch.device("cuda", 0)
    other = torch.int32 if dtype != torch.int32 else torch.int64
    yield "dtype", torch.zeros(shape, dtype=other, device=dev)
    yield "shape, one dimension more", torch.zeros(shape + (2,), dtype=dtype, device=dev)
    if not free or len(shape) > 1:
        yield "shape, last dimension", torch.zeros(shape[:-1] + (shape[-1] + 1,), dtype=dtype, device=dev)
    if not free:
        yield "shape, first dimension", torch.zeros((shape[0] + 1,) + shape[1:], dtype=dtype, device=dev)
    strided = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=dtype, device=dev)[..., ::2]
    assert tuple(strided.shape) == shape and not strided.is_contiguous()
    yield "a strided slice", strided
    if len(shape) > 1:
        transposed = torch.zeros(shape[:-2] + (shape[-1], shape[-2]), dtype=dtype, device=dev).transpose(-1, -2)
        assert tuple(transposed.shape) == shape and not transposed.is_contiguous()
        yield "a transposed view", transposed
    yield "on the CPU", torch.zeros(shape, dtype=dtype)


class _Duck:
    """anything with data_ptr / shape / dtype is taken by the step calls and copy_envs: a torch tensor's address under another shape"""

    def __init__(self, t, shape, dtype):
        self.t, self.shape, self.dtype = t, shape, dtype

    def data_ptr(self):
        return self.t.data_ptr()


@pytest.mark.gpu
def test_bad_tensors_are_refused_and_nothing_is_done(hip_lib):
    import torch
    with _handle() as env:
        before = env.get_state(), env.counters(), env.episodes()
        wrong = []
        rows = 0
        for call, arg, name, dtype, shape, free, fn in _table(env, torch):
            for what, t in _bad(torch, dtype, shape, free):
                rows += 1
                try:
                    fn(t)
                    wrong.append(f"{call} {arg}, {what}: accepted")
                except ValueError as e:
                    if name not in str(e):
                        wrong.append(f"{call} {arg}, {what}: the text does not name {name!r}: {e}")
                except Exception as e:  # noqa: BLE001 (every row is reported)
                    wrong.append(f"{call} {arg}, {what}: {type(e).__name__} instead of ValueError: {e}")
        # the duck-typed form of the older calls
        good = torch.zeros((N, 4), dtype=torch.int32, device=torch.device("cuda", 0))
        for what, duck in (("shape", _Duck(good, (N, 3), "int32")), ("dtype", _Duck(good, (N, 4), "int64")), ("no shape", _Duck(good, (), "int32"))):
            rows += 1
            try:
                env.step_device(duck)
                wrong.append(f"step_device duck-typed moves, {what}: accepted")
            except ValueError as e:
                if "moves" not in str(e):
                    wrong.append(f"step_device duck-typed moves, {what}: the text does not name 'moves': {e}")
        after = env.get_state(), env.counters(), env.episodes()
        assert after[0].tobytes() == before[0].tobytes(), "a refused call changed the state"
        assert np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2]), (before[1:], after[1:])
        assert rows > 100
        assert not wrong, f"{len(wrong)} of {rows} rows:\n" + "\n".join(wrong)


@pytest.mark.gpu
def test_step_device_raw_address_passes_unchecked_and_steps(hip_lib):
    import torch
    from pomcpp_amd.batch import CNT_STEPS
    with _handle() as env:
        state, cnt, running = env.get_state(), env.counters(), ~env.is_done()
        assert running.any()
        moves = torch.zeros((N, 4), dtype=torch.int32, device=torch.device("cuda", 0))
        torch.cuda.synchronize()   # a raw address is ordered by the caller
        env.step_device(moves.data_ptr())
        assert env.counters()[CNT_STEPS] == cnt[CNT_STEPS] + running.sum()
        assert np.array_equal(env.get_state()["timeStep"], state["timeStep"] + running)   # (a finished game is not stepped)
