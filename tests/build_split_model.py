"""The plan of the split sketch builder (selhip_build_sketches_split, csrc/host_plan.hpp: split_plan) in plain Python, nothing else.

The k-mer END positions of a genome of L codes are e in [k-1, L).  With a chunk length C chunk c owns
e in [k-1 + c C, min(k-1 + (c+1) C, L)); a genome has max(1, ceil((L - (k-1)) / C)) chunks and is split iff it has two.
The chunk's kernel sees codes[c C : c C + min(C + k-1, L - c C)]."""

SEG = 64                        # kernel_sketch.cuh: kSketchSeg
CHUNK_MIN = SEG * 1024          # host_plan.hpp: kSplitChunkMin
SCRATCH_MAX = 1 << 30           # host_plan.hpp: kSplitScratchMax
ROUNDS = 1                      # host_plan.hpp: kSplitRounds (w)
MERGE_SEGMENT = 64              # selection_hip.h: SELHIP_MERGE_SEGMENT
AUTO, OFF = 0, -1
MANY_ITEMS = 2048               # a launch of fewer items takes 1 024 threads per workgroup, else 256


def end_positions(L, k):
    return max(0, L - (k - 1))


def chunks_of(L, k, C):
    return max(1, -(-end_positions(L, k) // C)) if C > 0 else 1


def row_bytes(m, p_aux):
    return 16384 + 8 * m + ((1 << p_aux) if p_aux > 0 else 0)


def levels_of(c):
    if c < 2:
        return 0
    levels = 1
    while c > MERGE_SEGMENT:
        c = -(-c // MERGE_SEGMENT)
        levels += 1
    return levels


class Refused(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


def plan(lengths, k, m, p_aux, chunk, resident_blocks):
    """-> (info dict, chunks per genome); Refused("badarg") / Refused("nomem") as the library's statuses"""
    if chunk not in (AUTO, OFF) and (chunk < 0 or chunk % SEG):
        raise Refused("badarg")
    total = sum(end_positions(L, k) for L in lengths)
    C = 0 if chunk == OFF else chunk
    if chunk == AUTO:
        slots = ROUNDS * max(1, resident_blocks)
        per_slot = -(-total // slots)
        C = max(CHUNK_MIN, -(-per_slot // CHUNK_MIN) * CHUNK_MIN)
    while True:
        counts = [chunks_of(L, k, C) for L in lengths]
        split = [c for c in counts if c >= 2]
        if sum(split) * row_bytes(m, p_aux) <= SCRATCH_MAX:
            break
        if chunk != AUTO:
            raise Refused("nomem")
        C *= 2
    items = sum(split) + len(counts) - len(split)
    info = dict(chunk=C, items=items, split_genomes=len(split), chunks=sum(split), fallback_genomes=0,
                levels=levels_of(max(split, default=0)), threads=(1024 if items < MANY_ITEMS else 256) if lengths else 0)
    return info, counts


def items(lengths, k, C, counts):
    """the work items in launch order: (first code within the genome, codes, genome, kind); partial ones first, then the whole
    genomes, longest first (ties: input order)"""
    out = []
    for g, (L, c) in enumerate(zip(lengths, counts)):
        if c >= 2:
            out += [(j * C, min(C + k - 1, L - j * C), g, "partial") for j in range(c)]
    direct = [(0, L, g, "direct") for g, (L, c) in enumerate(zip(lengths, counts)) if c < 2]
    return out + sorted(direct, key=lambda it: -it[1])


def item_end_positions(item, k):
    """the end positions, in genome coordinates, that for_each_kmer visits on the item's sub-array: [k-1, len) of it"""
    start, length, _, _ = item
    return range(start + k - 1, start + length)


def needs_fallback(smh_row, m):
    """sketch_split_finish_kernel's test on the final buckets: a = max_b min(m-1, h[b] >> 32) > 0.  On the oracle's rows: a bucket
    that is empty or holds a value of a step beyond 0 is one that pass 0 alone could not have produced"""
    return max(min(m - 1, int(v) >> 32) for v in smh_row) > 0
