"""A call the library refuses (POM_E_ARG) names itself in pom_last_error() and has done nothing: the state bytes, the counters and the
episode numbers of the handle are what they were, and the handle goes on stepping like the oracle.

One handle of 20 envs, one whole tile and a short one (as tests/test_wrapper_args.py); nothing a refused call does reaches a kernel, so
no larger shape can fail differently.  The calls go to the library directly: the Python wrapper would refuse most of these itself."""
import ctypes as C

import numpy as np
import pytest

N, TICKS, SEED = 20, 5, 3


@pytest.mark.gpu
def test_refused_calls_name_themselves_and_do_nothing(hip_lib, oracle):
    import torch
    import pomcpp_amd as pa
    from pomcpp_amd.batch import BatchEnvironment, DIST_RANDOM, MODE_ENV, _ExpandSpec, _ViewSpec
    lib = hip_lib
    start = pa.make_boards(N, seed=5)
    dev = torch.device("cuda", 0)
    moves = torch.zeros((N, 4), dtype=torch.int32, device=dev)
    planes = torch.zeros((N, 16, 11, 11), dtype=torch.uint8, device=dev)
    idx = torch.arange(N, dtype=torch.int64, device=dev)
    host = np.zeros(N * 1004, dtype=np.uint8)         # room for any read-back of the batch
    idx_host = np.arange(N, dtype=np.int64)
    mv, pl, hp = moves.data_ptr(), planes.data_ptr(), host.ctypes.data
    view = _ViewSpec()
    view.struct_size, view.planes_dev, view.dtype, view.view_radius = C.sizeof(_ViewSpec), pl, 0, 4
    xs = _ExpandSpec()
    xs.struct_size, xs.first, xs.count, xs.src_dev, xs.moves_dev = C.sizeof(_ExpandSpec), 15, 11, idx.data_ptr(), mv
    with BatchEnvironment(N, device=0, mode=MODE_ENV, max_steps=800) as env:
        h = env._h
        env.make_game(start)
        env.step_random(SEED, DIST_RANDOM, ticks=TICKS)   # counters that are not zero
        before = env.get_state(), env.counters(), env.episodes()
        assert before[1].any()
        F, K = 15, 11                                     # the range [15, 26) of a batch of 20
        refused = [
            ("pom_batch_step", (h, None)),
            ("pom_batch_step_device", (h, None)),
            ("pom_batch_step_device_many", (h, None, 2)),
            ("pom_batch_step_device_many", (h, mv, -1)),
            ("pom_batch_step_random", (h, SEED, 3, 1, 1)),
            ("pom_batch_step_random", (h, SEED, DIST_RANDOM, 1, 0)),
            ("pom_batch_set_tick", (h, -1)),
            ("pom_batch_set_streams", (h, 0)),
            ("pom_batch_set_streams", (h, 9)),
            ("pom_batch_counters", (h, None)),
            ("pom_batch_counters_device", (h, None)),
            ("pom_batch_moves_device", (h, None)),
            ("pom_batch_stream", (h, None)),
            ("pom_batch_chain_stats", (h, None)),
            ("pom_batch_episodes", (h, 0, N, None)),
            ("pom_batch_policy_memory", (h, 0, N, None)),
            ("pom_batch_download", (h, None, 0, N)),
            ("pom_batch_upload", (h, None, 0, N)),
            # the range [15, 26) on every call that takes a range
            ("pom_batch_upload", (h, hp, F, K)),
            ("pom_batch_download", (h, hp, F, K)),
            ("pom_batch_download_terminal", (h, hp, F, K)),
            ("pom_batch_copy_envs", (h, idx_host.ctypes.data, F, K, 0)),
            ("pom_batch_copy_envs_device", (h, idx.data_ptr(), F, K, 0)),
            ("pom_batch_status", (h, F, K, hp, None, None, None, None, None)),
            ("pom_batch_last_results", (h, F, K, hp, None, None, None, None)),
            ("pom_batch_episodes", (h, F, K, hp)),
            ("pom_batch_policy_memory", (h, F, K, hp)),
            ("pom_batch_step_device_range", (h, F, K, mv, None, None, 0, 0, None, None)),
            ("pom_batch_step_device_range_view", (h, F, K, mv, None, None)),
            ("pom_batch_step_device_range_view", (h, F, K, mv, None, C.byref(view))),
            ("pom_batch_expand", (h, C.byref(xs))),
            ("pom_batch_observe", (h, None, 0, 0, None, None)),
            ("pom_batch_observe", (h, pl, 4, 0, None, None)),
        ]
        wrong = []
        for name, args in refused:
            assert lib.pom_batch_destroy(None) == 1       # another call's text stands in pom_last_error
            rc, text = getattr(lib, name)(*args), lib.pom_last_error().decode()
            if rc != 1 or not text.startswith(name + ": "):
                wrong.append((name, args[1:], rc, text))
        after = env.get_state(), env.counters(), env.episodes()
        assert not wrong, f"{len(wrong)} of {len(refused)}:\n" + "\n".join(map(str, wrong))
        assert after[0].tobytes() == before[0].tobytes(), "a refused call changed the state"
        assert np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2]), (before[1:], after[1:])
        # ... and the handle still steps like the oracle
        want = start.copy()
        oracle.run_random(want, start, TICKS, SEED, 0, 0, DIST_RANDOM, 800)
        want["agents"]["pad"] = 0
        assert after[0].tobytes() == want.tobytes()
        assert not env.is_done().any()                    # five ticks in: no bomb has gone off yet
        rng = np.random.default_rng(9)
        m = rng.integers(0, 6, size=(N, 4)).astype(np.int32)
        moves.copy_(torch.from_numpy(m))
        torch.cuda.synchronize()
        env.step_device(moves)
        for i in range(N):
            oracle.env_step(want[i:i + 1], m[i], dict(done=0, winner=-1, draw=0))
        want["agents"]["pad"] = 0
        assert env.get_state().tobytes() == want.tobytes(), "the step after the refusals differs from the oracle's"
