"""Several host threads at once: the crew that tests/test_threads_gpu.py and tests/threads_child.py run their threads in, and the guard
against a vacuous run (tests/test_threads_host.py pins both).  A plain helper module like tests/*_model.py; host only, no GPU call.

A crew is a fixed set of named threads.  What it promises:

  * an exception in one member is collected with its traceback and re-raised in the thread that called run(), together with every
    member's operation log;
  * the failing member breaks the barrier and sets the stop event; every member asks go() or meet() before each step and leaves through
    Halt, so that behind a failure -- a HIP error above all -- no member starts another call;
  * every barrier wait and every join has a time-out; a member that does not come back is reported (it is a daemon thread: it cannot
    be ended, and it does not keep the process alive);
  * a failure that names a HIP error is remembered for the process (hip_failed()): the tests that follow start nothing on the GPU.

timed(step, fn) stamps time.perf_counter() around fn; overlap(a, b) counts the steps of two members whose intervals intersect."""
import threading
import time
import traceback

TIMEOUT = 120.0                              # seconds: every barrier wait and every join
_HIP_FAILED = []                             # what a crew of this process met that names a HIP error (never cleared)


class Halt(Exception):
    """another member failed, or the crew was stopped: leave without another step"""


def hip_failed():
    """the first failure of this process that named a HIP error, or None"""
    return _HIP_FAILED[0] if _HIP_FAILED else None


def names_hip_error(exc):
    """a failed HIP call (SELHIP_E_HIP, torch's "HIP error"), or a wait that ran out -- a thread that sits in a call that does not return"""
    text = str(exc)
    return isinstance(exc, TimeoutError) or getattr(exc, "code", 0) == -2 or "HIP error" in text or "hipError" in text


class Member:
    """one thread of a crew: its name, its log (whatever the body appends) and its stamped intervals"""

    def __init__(self, crew, name):
        self.crew, self.name, self.log, self.spans = crew, name, [], {}

    def go(self):
        """in front of every step that waits for nobody"""
        if self.crew.stop.is_set():
            raise Halt

    def meet(self):
        """in front of every step that all members take together"""
        self.go()
        try:
            self.crew.barrier.wait()
        except threading.BrokenBarrierError:
            self.go()                                                 # (broken by a member that failed: the stop event was set first)
            raise TimeoutError(f"a barrier wait ran out after {self.crew.timeout} s: a member did not arrive") from None
        self.go()

    def timed(self, step, fn):
        t0 = time.perf_counter()
        try:
            return fn()
        finally:
            self.spans[step] = (t0, time.perf_counter())


class Crew:
    def __init__(self, names, timeout=TIMEOUT):
        self.members = {name: Member(self, name) for name in names}
        self.barrier = threading.Barrier(len(self.members), timeout=timeout)
        self.stop, self.timeout = threading.Event(), timeout
        self.errors, self._lock = [], threading.Lock()

    def _main(self, member, body):
        try:
            body(member)
        except Halt:
            pass
        except BaseException as e:                                   # noqa: BLE001  (collected, re-raised by run)
            with self._lock:
                self.errors.append((member.name, e, traceback.format_exc()))
                if names_hip_error(e):
                    _HIP_FAILED.append(f"{member.name}: {e}")
            self.halt()

    def halt(self):
        self.stop.set()
        self.barrier.abort()

    def logs(self, last=None):
        return "\n".join(f"  {m.name} ({len(m.log)} entries): {m.log if last is None else m.log[-last:]}" for m in self.members.values())

    def run(self, bodies):
        """bodies: {member name: body(member)}.  Returns when every thread has ended; raises what the first failing member raised, as
        an AssertionError that carries its traceback and every member's log"""
        assert set(bodies) == set(self.members)
        threads = [threading.Thread(target=self._main, args=(self.members[n], b), name=n, daemon=True) for n, b in bodies.items()]
        for t in threads:
            t.start()
        deadline = time.monotonic() + self.timeout
        for t in threads:
            t.join(max(0.0, deadline - time.monotonic()))
        stuck = [t.name for t in threads if t.is_alive()]
        if stuck:
            self.halt()
            for t in threads:
                t.join(5.0)
            _HIP_FAILED.append(f"threads {stuck} did not come back within {self.timeout} s")
            raise AssertionError(f"threads {stuck} did not come back within {self.timeout} s; errors so far: "
                                 f"{[(n, repr(e)) for n, e, _ in self.errors]}\n{self.logs()}")
        if self.errors:
            name, exc, tb = self.errors[0]
            others = "".join(f"\nalso thread {n}: {e!r}" for n, e, _ in self.errors[1:])
            raise AssertionError(f"thread {name}: {type(exc).__name__}: {exc}\n{tb}{others}\nthe logs of all threads:\n{self.logs()}") from exc

    def overlap(self, a, b):
        """(steps both members stamped, those whose two intervals intersect)"""
        sa, sb = self.members[a].spans, self.members[b].spans
        both = sorted(set(sa) & set(sb))
        return len(both), sum(1 for s in both if intersect(sa[s], sb[s]))


def intersect(x, y):
    return max(x[0], y[0]) < min(x[1], y[1])
