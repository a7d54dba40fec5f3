"""program.StepCache without a GPU: a Recorder works off the device and ``program.host_call`` closures stand in for launches.

A miss records, a hit refreshes the per-step inputs and then replays the closures in order; every key has its own program; a step
that marks its recorder invalid, or raises, files nothing; ``clear()`` drops the programs and keeps the counters."""
import pytest

from videosys_amd import program
from videosys_amd.program import StepCache


def stats(recorded, replayed, eager):
    return {"recorded": recorded, "replayed": replayed, "eager": eager}


def step(log, tag):
    """A ``record`` closure of two stand-in launches; its payload is ``tag``."""
    def record():
        program.host_call(lambda: log.append((tag, "first")))
        program.host_call(lambda: log.append((tag, "second")))
        return tag
    return record


def test_miss_records_hit_refreshes_then_replays_and_keys_are_apart():
    cache, log = StepCache(), []
    refresh = lambda payload: log.append(("refresh", payload))
    assert cache.stats == stats(0, 0, 0) and len(cache) == 0 and "a" not in cache
    assert cache.run("a", step(log, "A"), refresh) == "A"
    assert log == [("A", "first"), ("A", "second")], "a miss runs the step once, eagerly, without a refresh"
    assert cache.stats == stats(1, 0, 0) and "a" in cache and len(cache) == 1 and program.active() is None
    del log[:]
    never = lambda: pytest.fail("a hit must not record")
    assert cache.run("a", never, refresh) == "A"
    assert log == [("refresh", "A"), ("A", "first"), ("A", "second")], "a hit: one refresh, before the closures, which run in order"
    assert cache.stats == stats(1, 1, 0)
    del log[:]
    assert cache.run("b", step(log, "B")) == "B"                      # a second key records again
    assert log == [("B", "first"), ("B", "second")] and cache.stats == stats(2, 1, 0) and len(cache) == 2
    del log[:]
    assert cache.run("b", never) == "B" and cache.run("a", never, refresh) == "A"      # no refresh given: replay alone
    assert log == [("B", "first"), ("B", "second"), ("refresh", "A"), ("A", "first"), ("A", "second")]
    assert cache.stats == stats(2, 3, 0)
    # a filed program can be reached: what the tests and the bench tools read
    prog, payload = cache.entries["a"]
    assert payload == "A" and prog.n_launches == 0 and len(prog.segments) == 2


def test_unrecordable_step_files_nothing_and_counts_eager():
    cache, log = StepCache(), []

    def record():
        step(log, "A")()
        program.active().launch("vsys_no_such_entry_point", (), (), None)      # no op code: the recorder is invalid
        return "A"

    for n in (1, 2):                                                             # not remembered: it is tried again at every call
        assert cache.run("a", record) == "A"
        assert cache.stats == stats(0, 0, n) and "a" not in cache and len(cache) == 0 and program.active() is None
    assert log == [("A", "first"), ("A", "second")] * 2


def test_record_that_raises_leaves_no_recorder_and_an_empty_cache():
    cache = StepCache()

    def record():
        program.host_call(lambda: None)
        raise KeyError("launch error")

    with pytest.raises(KeyError, match="launch error"):
        cache.run("a", record)
    assert program.active() is None and len(cache) == 0 and cache.entries == {} and cache.stats == stats(0, 0, 0)
    assert cache.run("a", lambda: "A") == "A" and cache.stats == stats(1, 0, 0)   # the key is free to be recorded afterwards


def test_eager_counts_and_clear_keeps_the_counters():
    cache, log = StepCache(), []
    assert cache.eager(lambda: "out") == "out" and cache.stats == stats(0, 0, 1) and len(cache) == 0
    cache.run("a", step(log, "A"))
    cache.run("a", step(log, "A"))
    before = dict(cache.stats)
    assert before == stats(1, 1, 1)
    cache.clear()
    assert len(cache) == 0 and "a" not in cache and cache.stats == before
    cache.run("a", step(log, "A"))
    assert cache.stats == stats(2, 1, 1)


def test_stats_property_reads_and_assigns_the_cache_counters():
    class Owner:
        step_stats = program.stats_property("_steps")

        def __init__(self):
            self._steps = StepCache()

    o = Owner()
    o._steps.eager(lambda: None)
    assert o.step_stats == stats(0, 0, 1) and o.step_stats is o._steps.stats
    o.step_stats = stats(0, 0, 0)
    o._steps.run("a", lambda: None)
    assert o.step_stats == stats(1, 0, 0)
