"""-m "not gpu": the ORDER of PipelinedRunner's stream operations, pinned on the host.  Which stream waits for which event, where a
replay is enqueued, when the host arms and opens the common-start gate and when ``after`` runs are correct for measured reasons
(pipeline.py's comments) that only an MI355X can re-measure; this file keeps a refactoring of the class from moving any of them.

Nothing here needs a device: recording fakes stand in for torch.cuda.Stream / Event / stream / current_device, for
``pipe.capture`` (a callable that logs "replay slot s on <stream>"), for ops.new_workspaces (scripted poll / check results),
ops.lds_footprint and the gate launch (gnnpn_gate_wait; the word the gate polls logs the host's opening of it).  Streams and
events are numbered in order of creation, the slots' static inputs live on the meta device and "pinned" host arenas are ordinary
host tensors that say they are pinned.  Every scenario's log is compared with tests/golden/runner_schedule.json, which

    python tests/test_runner_schedule_host.py --record

rewrites from the pipeline.py in the tree (recorded from the class as it was before ``runner_plan`` / ``_enqueue`` / ``_wait`` /
``_load`` existed: the same file passes against both)."""
import contextlib
import json
import os
import sys
import types
import warnings

import pytest
import torch

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runner_schedule.json")
RUNNER_ENV = ("GNNPN_PIPE_HALVES", "GNNPN_PIPE_STREAM_PRIORITY", "GPU_MAX_HW_QUEUES", "GNNPN_PIPE_DECODE_IMPL", "GNNPN_SLOT_LDS_KB",
              "GNNPN_PIPE_FRONT_LDS_KB", "GNNPN_PIPE_LOCKSTEP", "GNNPN_PIPE_COMMON_START_US")


class Harness:
    """The fakes, installed with ``monkeypatch``, and the log they write."""

    def __init__(self, monkeypatch, env=None):
        from gnnpn_sc_amd import _lib, ops, pipeline
        self.pipeline, self.ops = pipeline, ops
        self.log, self.current, self.workspaces = [], [], []
        self.n_streams = self.n_events = 0
        self.finished = False                      # what every event's query() answers (lockstep: has the leader finished?)
        h = self
        for name in RUNNER_ENV:
            monkeypatch.delenv(name, raising=False)
        for name, value in (env or {}).items():
            monkeypatch.setenv(name, value)
        monkeypatch.setattr(pipeline, "_last_runner_on_device", {})
        monkeypatch.setattr(pipeline, "HOST_COPY_ON_ITS_OWN_STREAM", True)
        monkeypatch.setattr(pipeline, "DEFAULT_WRITE_THROUGH", False)

        class Stream:
            def __init__(self, device=None, priority=0):
                self.name = f"s{h.n_streams}"
                h.n_streams += 1
                h.log.append(f"{self.name} = Stream(priority={priority})")

            def wait_event(self, ev):
                h.log.append(f"{self.name}.wait_event({ev.name})")

            def wait_stream(self, other):
                h.log.append(f"{self.name}.wait_stream({other.name})")

            def synchronize(self):
                h.log.append(f"{self.name}.synchronize()")

        class Event:
            def __init__(self, *a, **k):
                self.name = f"e{h.n_events}"
                h.n_events += 1

            def record(self, stream=None):
                h.log.append(f"{self.name}.record({stream.name if stream is not None else h.where()})")

            def query(self):
                return h.finished

        @contextlib.contextmanager
        def stream(st):
            h.current.append(st)
            try:
                yield
            finally:
                h.current.pop()

        class Workspaces:
            def __init__(self, device):
                self.name, self.poll_script, self.check_script, self.last_progress = f"ws{len(h.workspaces)}", [], [], None
                h.workspaces.append(self)

            def poll(self):
                word = self.poll_script.pop(0) if self.poll_script else 0
                h.log.append(f"{self.name}.poll() -> {word:#x}")
                return word

            def check(self, what="cooperative kernel"):
                word = self.check_script.pop(0) if self.check_script else 0
                h.log.append(f"{self.name}.check() -> {word:#x}")
                if word:
                    err = ops.GnnpnError(f"{what}: status {word:#x}")
                    err.status = word
                    raise err

        class lds_footprint:
            def __init__(self, kb):
                self.kb = kb

            def __enter__(self):
                h.log.append(f"lds_footprint({self.kb})")

            def __exit__(self, *exc):
                return False

        class GateFlag:                            # the pinned word gnnpn_gate_wait polls: the host opens the gate by writing it
            def data_ptr(self):
                return 0

            def __setitem__(self, i, v):
                h.log.append(f"gate opened (seq {v})")

        def gate_wait(flag, seq, us, st):
            h.log.append(f"gate armed (seq {seq}, {us} us) on {h.where()}")
            return 0

        real_empty, real_copy = torch.empty, torch.Tensor.copy_

        def empty(*a, pin_memory=False, **k):
            t = real_empty(*a, **k)
            t.says_pinned = bool(pin_memory)
            return t

        def copy_(self, src, non_blocking=False):
            if h.current:                          # inside a ``with torch.cuda.stream(..)``: a copy of submit's, not of _clone's
                h.log.append(f"copy on {h.where()}")
            return real_copy(self, src, non_blocking)

        monkeypatch.setattr(torch.cuda, "Stream", Stream)
        monkeypatch.setattr(torch.cuda, "Event", Event)
        monkeypatch.setattr(torch.cuda, "stream", stream)
        monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
        monkeypatch.setattr(torch, "empty", empty)
        monkeypatch.setattr(torch.Tensor, "copy_", copy_)
        monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: GateFlag())
        monkeypatch.setattr(torch.Tensor, "is_pinned", lambda self, *a, **k: getattr(self, "says_pinned", False))
        monkeypatch.setattr(ops, "new_workspaces", Workspaces)
        monkeypatch.setattr(ops, "lds_footprint", lds_footprint)
        monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(gnnpn_gate_wait=gate_wait))
        monkeypatch.setattr(_lib, "stream_ptr", lambda: None)

    def where(self):
        return self.current[-1].name if self.current else "the default stream"

    def pipe(self, precision="split", seq_len=235):
        h, slots = self, []

        def capture(services, batch, warmup=2, decode_impl=0, lds_kb=0, ws=None, paired_start=False, pool=None, write_through=False):
            if not any(b is batch for b in slots):
                slots.append(batch)
            s = [i for i, b in enumerate(slots) if b is batch][0]
            names = [w.name for w in (ws if isinstance(ws, (tuple, list)) else [ws])]
            h.log.append(f"capture slot {s}: decode_impl={decode_impl} lds_kb={lds_kb} ws={'+'.join(names)} "
                         f"paired_start={paired_start} write_through={write_through}")
            outputs = {"slot": s}

            def replay():
                h.log.append(f"replay slot {s} on {h.where()}")
                return outputs
            replay.outputs = outputs
            return replay
        return types.SimpleNamespace(precision=precision, capture=capture,
                                     low=types.SimpleNamespace(actor=types.SimpleNamespace(seq_len=seq_len)))

    def batch(self, n_problems=48, device="meta", max_nodes=0, n_tasks=3):
        from gnnpn_sc_amd import graph
        n, e = 2 * n_problems, 3 * n_problems

        def t(shape, dtype):
            return torch.zeros(shape, dtype=dtype, device=device)
        return self.pipeline.DeviceBatch(t((n, 7), torch.float32), graph.CSR(t((n + 1,), torch.int32), t((e,), torch.int32), None, n),
                                         t((n_problems + 1,), torch.int32), t((n_problems, n_tasks, 4), torch.float64),
                                         t((n_problems, n_tasks), torch.uint8), t((n_problems, 4), torch.float64), max_nodes)

    def runner(self, slots=2, n_problems=48, precision="split", seq_len=235, **kw):
        return self.pipeline.PipelinedRunner(self.pipe(precision, seq_len), None, self.batch(n_problems), slots=slots, **kw)

    def after(self, out, slot):
        self.log.append(f"after(slot {slot}, outputs of slot {out['slot']}) on {self.where()}")

    def submit(self, runner, batch=None, note=""):
        self.log.append(f"-- submit{note}")
        out, slot = runner.submit(batch, after=self.after)
        self.log.append(f"-> slot {slot}, outputs of slot {out['slot']}")

    def call(self, what, fn):
        self.log.append(f"-- {what}")
        return fn()


@contextlib.contextmanager
def warnings_logged(h):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        yield
    for w in caught:
        h.log.append(f"{w.category.__name__}: {str(w.message).split(';')[0]}")


def two_free_running_slots(h):
    runner = h.runner(slots=2)
    packed = [runner.pack(h.batch()) for _ in range(2)]
    for i in range(5):
        h.submit(runner, packed[i % 2])
    h.call("synchronize", runner.synchronize)


def resident_and_unpacked_batches(h):
    runner = h.runner(slots=2)
    h.submit(runner, None, " of the resident batch")
    h.submit(runner, h.batch(), " of a batch that is not packed")
    h.submit(runner, runner.pack_host(h.batch(device="cpu")), " of a pinned host arena")
    h.submit(runner, runner.pack_host(h.batch(device="cpu")), " of a pinned host arena")
    h.submit(runner, runner.pack_host(h.batch(device="cpu")), " of a pinned host arena")
    h.call("poll", runner.poll)


def halves_two_slots_on_one_stream(h):
    runner = h.runner(slots=2, n_problems=512)
    assert runner.halves and len(runner.streams) == 1
    packed = runner.pack(h.batch(512))
    host = runner.pack_host(h.batch(512, device="cpu"))
    for i in range(4):
        h.submit(runner, packed)
    for i in range(3):
        h.submit(runner, host, " of a pinned host arena")
    h.call("synchronize", runner.synchronize)


def three_slots_on_two_streams(h):
    runner = h.runner(slots=3)
    packed = runner.pack(h.batch())
    for i in range(7):
        h.submit(runner, packed)
    h.call("synchronize", runner.synchronize)


def lockstep_pairs(h):
    runner = h.runner(slots=2, seq_len=2000)
    assert runner.lockstep
    packed = runner.pack(h.batch())
    h.finished = False
    h.submit(runner, packed, ": leads")
    h.submit(runner, packed, ", the leader has not finished: joins it")
    h.submit(runner, packed, ": leads")
    h.finished = True
    h.submit(runner, packed, ", the leader has finished: leads")
    h.submit(runner, packed, ", the leader has finished: leads")
    h.finished = False
    h.submit(runner, packed, ", the leader has not finished: joins it")
    h.call("synchronize", runner.synchronize)


def lockstep_with_staged_host_batches(h):
    runner = h.runner(slots=2, seq_len=2000)
    host = [runner.pack_host(h.batch(device="cpu")) for _ in range(2)]
    h.submit(runner, host[0], ": the leader is deferred")
    assert runner._deferred is not None
    h.submit(runner, host[1], ": the pair is enqueued together")
    assert runner._deferred is None
    h.submit(runner, host[0], ": the leader is deferred")
    h.submit(runner, host[1], ": the pair is enqueued together")
    h.submit(runner, host[0], ": the leader is deferred")
    h.call("stream(0) flushes the waiting leader alone", lambda: runner.stream(0))
    assert runner._deferred is None
    h.submit(runner, host[1], ": the leader is deferred")
    h.call("poll flushes the waiting leader alone", runner.poll)
    assert runner._deferred is None
    h.submit(runner, host[0], ": the leader is deferred")
    h.submit(runner, None, " of the resident batch: the waiting leader goes first, alone")
    h.submit(runner, host[0], ": the leader is deferred")
    h.call("synchronize flushes the waiting leader alone", runner.synchronize)


def common_start_of_a_burst(h):
    runner = h.runner(slots=2)
    assert runner.common_start_us == 400 and runner._drained and runner._gate is None
    packed = runner.pack(h.batch())
    for i in range(5):
        h.submit(runner, packed, f" {i + 1} of a burst of five")
        assert (runner._gate is not None) == (i == 0) and not runner._drained
    h.call("synchronize", runner.synchronize)
    assert runner._drained
    for i in range(4):
        h.submit(runner, packed, f" {i + 1} of a burst of four")
    h.call("poll", runner.poll)
    h.submit(runner, packed, ": a burst of one")
    assert runner._gate is not None
    h.call("stream(0) leaves the gate pending", lambda: runner.stream(0))
    assert runner._gate is not None
    h.call("poll opens it", runner.poll)
    assert runner._gate is None and runner._drained
    host = runner.pack_host(h.batch(device="cpu"))
    for i in range(2):
        h.submit(runner, host, " of a pinned host arena: not held")
        assert runner._gate is None and not runner._drained
    h.call("synchronize", runner.synchronize)


def two_runners_take_turns(h):
    a, b = h.runner(slots=2), h.runner(slots=2)
    for note, r in (("a", a), ("a", a), ("b", b), ("b", b), ("a", a), ("b", b)):
        h.submit(r, None, f" to runner {note}")
    h.call("synchronize a", a.synchronize)
    h.call("synchronize b", b.synchronize)


def two_runners_with_a_held_burst(h):
    a, b = h.runner(slots=2), h.runner(slots=2, seq_len=2000)
    h.submit(a, None, " to runner a: held behind the gate")
    h.submit(b, b.pack_host(h.batch(device="cpu")), " to runner b: its leader is deferred")
    h.submit(a, None, " to runner a: b's leader goes first")
    h.submit(b, None, " to runner b: a's gate is opened first")
    h.call("synchronize a", a.synchronize)
    h.call("synchronize b", b.synchronize)


def degrade_at_poll(h):
    runner = h.runner(slots=2, write_through=False)
    for i in range(3):
        h.submit(runner, None)
    h.workspaces[1].poll_script.append(0x10)
    with warnings_logged(h):
        word = h.call("poll finds status 0x10", runner.poll)
    assert word == 0x10 and runner.degraded == 0x10 and runner.write_through
    assert runner._gate is None and runner._drained and runner._deferred is None and runner._open_leader is None
    assert runner._last_done == [None, None] and runner._slot_done == [None, None]
    for i in range(3):
        h.submit(runner, None)
    h.workspaces[0].poll_script.append(0x3)
    with warnings_logged(h):
        assert h.call("poll finds status 0x3: nothing left to switch to", runner.poll) == 0x3
    assert runner.degraded == 0x10
    h.call("synchronize", runner.synchronize)


def degrade_at_synchronize(h):
    runner = h.runner(slots=2, seq_len=2000)
    host = runner.pack_host(h.batch(device="cpu"))
    for i in range(3):
        h.submit(runner, host)
    for w in h.workspaces:
        w.check_script.append(0x2)
    with warnings_logged(h), pytest.raises(h.ops.GnnpnError, match="status 0x2"):
        h.call("synchronize finds status 0x2 in both workspaces", runner.synchronize)
    assert runner.degraded == 0x2 and runner.write_through
    assert runner._gate is None and runner._drained and runner._deferred is None and runner._open_leader is None
    assert runner._last_done == [None, None] and runner._slot_done == [None, None]
    for i in range(2):
        h.submit(runner, host)
    h.call("synchronize without check", lambda: runner.synchronize(check=False))
    frozen = h.runner(slots=2, auto_degrade=False)
    h.submit(frozen, None)
    h.workspaces[2].poll_script.append(0x10)
    with warnings_logged(h):
        assert h.call("poll of a runner without auto_degrade", frozen.poll) == 0x10
    assert frozen.degraded is None and not frozen.write_through


SCENARIOS = {
    "two_free_running_slots": (two_free_running_slots, {}),
    "resident_and_unpacked_batches": (resident_and_unpacked_batches, {}),
    "halves_two_slots_on_one_stream": (halves_two_slots_on_one_stream, {}),
    "three_slots_on_two_streams": (three_slots_on_two_streams, {}),
    "lockstep_pairs": (lockstep_pairs, {}),
    "lockstep_with_staged_host_batches": (lockstep_with_staged_host_batches, {}),
    "common_start_of_a_burst": (common_start_of_a_burst, {"GNNPN_PIPE_COMMON_START_US": "400"}),
    "two_runners_take_turns": (two_runners_take_turns, {}),
    "two_runners_with_a_held_burst": (two_runners_with_a_held_burst, {"GNNPN_PIPE_COMMON_START_US": "400"}),
    "degrade_at_poll": (degrade_at_poll, {}),
    "degrade_at_synchronize": (degrade_at_synchronize, {}),
}


def run_scenario(name, monkeypatch):
    fn, env = SCENARIOS[name]
    h = Harness(monkeypatch, env)
    fn(h)
    return h.log


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_schedule_matches_the_recorded_one(name, monkeypatch):
    with open(GOLDEN_FILE) as f:
        expected = json.load(f)[name]
    got = run_scenario(name, monkeypatch)
    for i, (g, e) in enumerate(zip(got, expected)):
        assert g == e, f"{name}: operation {i} is {g!r}, recorded {e!r} (after {got[max(0, i - 3):i]})"
    assert len(got) == len(expected), f"{name}: {len(got)} operations, recorded {len(expected)}"


def test_submit_refuses_a_batch_the_captured_graph_cannot_take(monkeypatch):
    """``submit``'s two refusals: a batch of large workflow graphs for a graph that holds the one-launch GIN branch, and an
    unpacked batch of other shapes."""
    h = Harness(monkeypatch)
    runner = h.pipeline.PipelinedRunner(h.pipe(), None, h.batch(max_nodes=4), slots=2)
    with pytest.raises(h.ops.GnnpnError, match="max_nodes = 0"):
        runner.submit(h.batch(max_nodes=0))
    with pytest.raises(h.ops.GnnpnError, match="max_nodes = 17"):
        runner.submit(runner.pack(h.batch(max_nodes=h.ops.REQUEST_BRANCH_MAX_NODES + 1)))
    with pytest.raises(h.ops.GnnpnError, match="batch shape"):
        runner.submit(h.batch(n_problems=32, max_nodes=4))
    runner.submit(h.batch(max_nodes=h.ops.REQUEST_BRANCH_MAX_NODES))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    recorded = {}
    for scenario in SCENARIOS:
        with pytest.MonkeyPatch.context() as mp:
            recorded[scenario] = run_scenario(scenario, mp)
    with open(GOLDEN_FILE, "w") as f:
        json.dump(recorded, f, indent=0)
        f.write("\n")
    sys.path.insert(0, os.path.dirname(GOLDEN_FILE))
    import manifest                                # tests/golden/MANIFEST.json: every fixture as its generator wrote it
    manifest.update()
    print({k: len(v) for k, v in recorded.items()})
