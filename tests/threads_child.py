"""Run by tests/test_threads_gpu.py as a fresh child process: the FIRST calls of selhip_synth_generate, selhip_build_sketches,
selhip_build_sketches_split and selhip_linkage of a process, made by three threads at once.  Each of the first three raises its kernel's
dynamic LDS limit in a std::call_once (csrc/abi_blocks.inc, csrc/host_build.hpp); a thread that got past the flag before the attribute
stood would launch a kernel that asks for more LDS than it may.  selhip_linkage has no such flag: its first calls load its kernels and
take their per-call scratch side by side.  Every thread has its own stream and inputs (three seeds); what it gets is compared with the
generator's host twin, the builder's oracle and the linkage model (tests/thread_entries.py), computed before the first device call.

Prints "threads_child ok" and exits 0, or prints the failure and exits 1.  Not a test module: pytest does not collect it."""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))


def main():
    import torch

    import stream_harness as H
    import thread_entries as E
    import thread_harness as T

    sets = [E.bare_set(f"child{t}", 0xC41D0000 + 17 * t, m=(64, 128, 256)[t], p_aux=(6, 8, 10)[t]) for t in range(3)]
    for S in sets:                                                   # (host only: the generator's twin, the builder's oracle, the model)
        S.block_synth, S.block_build, S.block_linkage
    streams = []
    while len(streams) < 3:
        s = torch.cuda.Stream()
        if all(s.cuda_stream != o.cuda_stream for o in streams):
            streams.append(s)
    names = [S.name for S in sets]
    crew = T.Crew(names, timeout=90.0)

    def body(t):
        S, st = sets[t], streams[t]

        def run(me):
            with torch.cuda.stream(st):
                torch.zeros(16, device="cuda").add_(1.0).cpu()      # (this thread's first device work is torch's, not the library's)
                for name in E.FIRST_CALLS:
                    me.meet()
                    me.log.append(name)
                    got, want = me.timed(name, lambda: E.ENTRIES[name](S, st))
                    assert H.same(got, want), f"{name} on {S.name}: {H.describe(got, want)}"
        return run
    try:
        crew.run({names[t]: body(t) for t in range(3)})
    except AssertionError as e:
        print(e)
        return 1
    torch.cuda.synchronize()
    for name in E.FIRST_CALLS:
        spans = [crew.members[n].spans[name] for n in names]
        print(f"{name}: first calls {[f'{(a - spans[0][0]) * 1e3:.2f}..{(b - spans[0][0]) * 1e3:.2f} ms' for a, b in spans]}")
    print("threads_child ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
