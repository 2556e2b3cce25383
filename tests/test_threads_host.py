"""tests/thread_harness.py on the CPU: what tests/test_threads_gpu.py relies on when a thread fails, and how it counts overlap.  A crew
that swallowed a failure, let the other threads run on behind it, or counted threads that ran one after the other as running side by
side would make every test built on it vacuous.  No GPU; the waits are events, nothing sleeps."""
import threading

import pytest

import thread_harness as T


def test_a_failure_is_raised_with_every_log_and_stops_the_others():
    crew = T.Crew(["A", "B", "C"], timeout=20.0)
    steps = {"B": 0, "C": 0}
    before = len(T._HIP_FAILED)

    def failing(me):
        me.log.append("a0")
        me.meet()
        me.log.append("a1")
        raise ValueError("boom in A")

    def follower(me):
        me.log.append(me.name + "0")
        me.meet()
        while True:                                                  # (ends through Halt: the failing member broke the barrier)
            me.meet()
            steps[me.name] += 1
    with pytest.raises(AssertionError) as e:
        crew.run({"A": failing, "B": follower, "C": follower})
    text = str(e.value)
    assert "thread A: ValueError: boom in A" in text and "Traceback" in text
    assert "['a0', 'a1']" in text and "['B0']" in text and "['C0']" in text, text
    assert crew.stop.is_set() and steps == {"B": 0, "C": 0}, "nobody took another step behind the failure"
    assert isinstance(e.value.__cause__, ValueError)
    assert len(T._HIP_FAILED) == before, "a plain failure does not close the GPU for the tests that follow"


def test_free_running_members_stop_at_their_next_step():
    crew = T.Crew(["A", "B"], timeout=20.0)
    failed, taken = threading.Event(), []

    def failing(me):
        me.meet()
        try:
            raise AssertionError("wrong answer")
        finally:
            failed.set()

    def walker(me):
        me.meet()
        assert failed.wait(20.0)
        assert crew.stop.wait(20.0)                                  # (the crew sets it right behind the failure)
        me.go()
        taken.append("a step behind the failure")
    with pytest.raises(AssertionError, match="wrong answer"):
        crew.run({"A": failing, "B": walker})
    assert not taken


def test_a_wait_that_ran_out_is_a_failure():
    """a barrier whose wait ran out breaks itself, with the stop event unset (simulated by abort(): nothing here waits for a time limit):
    the members that were waiting fail, they do not leave quietly"""
    crew = T.Crew(["A", "B"], timeout=20.0)
    before = len(T._HIP_FAILED)
    try:
        with pytest.raises(AssertionError, match="a barrier wait ran out"):
            crew.run({"A": lambda me: me.meet(), "B": lambda me: crew.barrier.abort()})
        assert len(T._HIP_FAILED) == before + 1, "a thread that does not come back closes the GPU for the tests that follow"
    finally:
        del T._HIP_FAILED[before:]


def test_names_hip_error():
    from cuda_selection_criteria_amd import SelhipError
    assert T.names_hip_error(SelhipError(-2, "hipMemcpyAsync(...) failed: an illegal memory access was encountered"))
    assert T.names_hip_error(RuntimeError("HIP error: invalid device function")) and T.names_hip_error(TimeoutError("a barrier wait ran out"))
    assert not T.names_hip_error(SelhipError(-1, "unknown parameter 'x'")) and not T.names_hip_error(AssertionError("smh_a-sig on BIG: got (3,), want (4,)"))


def test_overlap_counts_intersecting_intervals_only():
    crew = T.Crew(["A", "B"])
    a, b = crew.members["A"], crew.members["B"]
    a.spans = {0: (0.0, 1.0), 1: (2.0, 3.0), 2: (4.0, 5.0), 3: (6.0, 7.0), 9: (8.0, 9.0)}
    b.spans = {0: (0.5, 0.6), 1: (3.0, 3.5), 2: (3.5, 4.5), 3: (7.5, 8.0), 8: (8.0, 9.0)}
    assert crew.overlap("A", "B") == (4, 2), "inside and straddling count; touching ends and disjoint intervals do not; steps of one member alone are left out"


def test_timed_stamps_around_the_call_also_when_it_raises():
    crew = T.Crew(["A"])
    me = crew.members["A"]
    assert me.timed("ok", lambda: 5) == 5
    with pytest.raises(KeyError):
        me.timed("bad", lambda: {}["x"])
    assert set(me.spans) == {"ok", "bad"} and all(t0 <= t1 for t0, t1 in me.spans.values())
