"""-m "not gpu": pipeline.runner_plan, the mode of a PipelinedRunner as a pure function of the batch size, the slots, the precision,
the recurrence length, the constructor's arguments and an environment given as a dict.  The expected values are what
PipelinedRunner.__init__ decided inline before the function existed (COMMON_START_US == 0, the default)."""
import pytest

from gnnpn_sc_amd import ops, pipeline
from gnnpn_sc_amd.pipeline import RunnerPlan, runner_plan


def plan(n_problems=48, slots=2, precision="split", seq_len=235, env=None, **kw):
    return runner_plan(n_problems, slots, precision, seq_len, env=dict(env or {}), **kw)


def fields(p, *names):
    return tuple(getattr(p, n) for n in names)


MODE = ("halves", "n_streams", "n_workspaces", "decode_impl", "lds_kb", "front_lds_kb", "lockstep", "common_start_us")


def test_defaults_this_table_was_read_at():
    assert pipeline.COMMON_START_US == 0


def test_two_free_running_slots():
    p = plan()
    assert isinstance(p, RunnerPlan) and p.n_slots == 2
    assert fields(p, *MODE) == (False, 2, 2, 4, (78, 78), 78, False, 0.0)
    assert p.stream_priority == 0 and p.priority_chosen is True
    f32 = plan(precision="f32")
    assert f32.lds_kb == (0, 0) and f32.front_lds_kb == 0
    assert fields(f32, *MODE) == (False, 2, 2, 4, (0, 0), 0, False, 0.0)


def test_half_batches_from_512_problems():
    assert fields(plan(512), *MODE) == (True, 1, 2, 4, (78, 78), 0, False, 0.0)
    assert plan(511).halves is False
    two_streams = plan(512, halves=False)
    assert fields(two_streams, *MODE) == (False, 2, 2, 4, (78, 78), 78, False, 0.0)
    assert plan(512, env={"GNNPN_PIPE_HALVES": "0"}) == two_streams
    assert plan(512, env={"GNNPN_PIPE_HALVES": "1"}).halves is True
    assert plan(512, halves=True, env={"GNNPN_PIPE_HALVES": "0"}).halves is True        # the argument wins


def test_one_slot():
    for precision in ("split", "f32"):
        p = plan(4096, slots=1, precision=precision)
        assert p.n_slots == 1 and fields(p, *MODE) == (False, 1, 1, 0, (0,), 0, False, 0.0)
    assert plan(4096, slots=0).n_slots == 1
    p = plan(4096, slots=1, halves=True)
    assert fields(p, "halves", "n_streams", "n_workspaces", "decode_impl") == (True, 1, 2, 4) and p.lds_kb == (78,)


@pytest.mark.parametrize("seq_len", [235, 2000])
@pytest.mark.parametrize("lockstep", [None, "0", "1"])
def test_three_slots(seq_len, lockstep):
    env = {"GNNPN_PIPE_COMMON_START_US": "400"}
    if lockstep is not None:
        env["GNNPN_PIPE_LOCKSTEP"] = lockstep
    p = plan(slots=3, seq_len=seq_len, env=env)
    assert p.n_slots == 3 and fields(p, *MODE) == (False, 2, 3, 4, (78, 78, 78), 78, False, 0.0)


def test_lockstep():
    p = plan(seq_len=2000, env={"GNNPN_PIPE_COMMON_START_US": "400"})
    assert p.lockstep is True and p.common_start_us == 0.0
    assert plan(seq_len=1999).lockstep is False
    assert plan(seq_len=2000, env={"GNNPN_PIPE_LOCKSTEP": "0"}).lockstep is False
    assert plan(seq_len=235, env={"GNNPN_PIPE_LOCKSTEP": "1"}).lockstep is True
    assert plan(512, seq_len=2000).lockstep is False                      # half-batches: one stream
    assert plan(512, seq_len=2000, env={"GNNPN_PIPE_LOCKSTEP": "1"}).lockstep is False
    assert plan(slots=1, seq_len=2000).lockstep is False


def test_common_start():
    env = {"GNNPN_PIPE_COMMON_START_US": "400"}
    p = plan(env=env)
    assert p.common_start_us == 400.0 and p.lockstep is False
    assert plan(seq_len=2000, env={**env, "GNNPN_PIPE_LOCKSTEP": "0"}).common_start_us == 400.0
    assert plan(512, env=env).common_start_us == 0.0
    assert plan(slots=1, env=env).common_start_us == 0.0


def test_stream_priority():
    p = plan(collective_stream=True)
    assert p.stream_priority == -1 and p.priority_chosen is True
    assert plan(collective_stream=True, env={"GPU_MAX_HW_QUEUES": "8"}).stream_priority == 0
    assert plan(collective_stream=True, env={"GPU_MAX_HW_QUEUES": "7"}).stream_priority == -1
    assert plan(collective_stream=True, env={"GPU_MAX_HW_QUEUES": ""}).stream_priority == -1      # empty reads as 4
    assert plan(512, collective_stream=True).stream_priority == 0                                 # half-batches: one stream
    assert plan(slots=1, collective_stream=True).stream_priority == 0
    assert plan(slots=3, collective_stream=True).stream_priority == -1
    p = plan(env={"GNNPN_PIPE_STREAM_PRIORITY": "-1"})
    assert p.stream_priority == -1 and p.priority_chosen is False
    p = plan(stream_priority=0, collective_stream=True, env={"GNNPN_PIPE_STREAM_PRIORITY": "-1"})
    assert p.stream_priority == 0 and p.priority_chosen is False
    p = plan(stream_priority=-1)
    assert p.stream_priority == -1 and p.priority_chosen is False


def test_hardware_queue_count_is_read_in_one_place():
    assert pipeline._hw_queues({}) == 4 and pipeline._hw_queues({"GPU_MAX_HW_QUEUES": ""}) == 4
    assert pipeline._hw_queues({"GPU_MAX_HW_QUEUES": "32"}) == 32


def test_overrides():
    assert plan(env={"GNNPN_PIPE_DECODE_IMPL": "3"}).decode_impl == 3
    assert plan(slots=1, env={"GNNPN_PIPE_DECODE_IMPL": "3"}).decode_impl == 3
    p = plan(env={"GNNPN_SLOT_LDS_KB": "100,56"})
    assert p.lds_kb == (100, 56) and p.front_lds_kb == 78
    assert plan(env={"GNNPN_SLOT_LDS_KB": ""}).lds_kb == (78, 78)          # empty: unset
    assert plan(env={"GNNPN_PIPE_FRONT_LDS_KB": "0"}).front_lds_kb == 0
    assert plan(512, env={"GNNPN_PIPE_FRONT_LDS_KB": "64"}).front_lds_kb == 64


def test_write_through(monkeypatch):
    assert plan().write_through is pipeline.DEFAULT_WRITE_THROUGH
    assert plan(write_through=True).write_through is True and plan(write_through=0).write_through is False
    monkeypatch.setattr(pipeline, "DEFAULT_WRITE_THROUGH", True)
    assert plan().write_through is True and plan(write_through=False).write_through is False


def test_a_footprint_list_shorter_than_the_slots_is_refused():
    with pytest.raises(ops.GnnpnError, match=r"GNNPN_SLOT_LDS_KB.* 1 entr.* 2 slots"):
        plan(env={"GNNPN_SLOT_LDS_KB": "100"})
    with pytest.raises(ops.GnnpnError, match=r"GNNPN_SLOT_LDS_KB.* 2 entr.* 3 slots"):
        plan(slots=3, env={"GNNPN_SLOT_LDS_KB": "100,56"})
    assert plan(slots=1, env={"GNNPN_SLOT_LDS_KB": "100"}).lds_kb == (100,)


def test_the_plan_reads_nothing_but_its_arguments(monkeypatch):
    """The process's own environment is only the default of ``env``."""
    for name, value in (("GNNPN_PIPE_HALVES", "0"), ("GNNPN_PIPE_DECODE_IMPL", "3"), ("GNNPN_SLOT_LDS_KB", "1,2"), ("GNNPN_PIPE_LOCKSTEP", "1"),
                        ("GNNPN_PIPE_STREAM_PRIORITY", "-1"), ("GNNPN_PIPE_FRONT_LDS_KB", "5"), ("GNNPN_PIPE_COMMON_START_US", "400"),
                        ("GPU_MAX_HW_QUEUES", "8")):
        monkeypatch.setenv(name, value)
    assert plan(512) == RunnerPlan(n_slots=2, halves=True, n_streams=1, n_workspaces=2, stream_priority=0, priority_chosen=True,
                                   decode_impl=4, lds_kb=(78, 78), front_lds_kb=0, lockstep=False, common_start_us=0.0,
                                   write_through=pipeline.DEFAULT_WRITE_THROUGH)
    p = runner_plan(512, 2, "split", 235, collective_stream=True)
    assert fields(p, *MODE) == (False, 2, 2, 3, (1, 2), 5, True, 0.0) and p.stream_priority == -1 and p.priority_chosen is False
    with pytest.raises(Exception):
        p.halves = True                                                    # frozen
