"""CPU checker of fgpu_pair_weights (no GPU, no engine import): the rules of include/fgpu.h restated in plain Python / numpy.

pair_weights(n, rels, attr, flags, active=None, missing=1.0) -> (rows, cols, bits, kept, stats)
    rels: the EFFECTIVE relationships (type, src, dst, id) of the selected tensors, as Tensor::iter_edges gives them (a dp value
    has won over m's, a dm entry has hidden m's, a multi-edge pair is one tuple per id).  A tuple given twice is one tuple, as a
    type given twice is one type.  attr: None (every relationship weighs 1.0; bits is then None: W is a BOOL pattern), or
    {id: float} — an id that is not a key weighs `missing`.  flags: the FGPU_PAIRS_* bits.  active: None or bool[n].
    The result is sorted by (row, col): W's binary64 bit patterns, K's kept ids, and the eight stats.  A refused weight raises
    Refused, its `id` the smallest refused relationship id.  The order of weights is msf_check.key_of."""
import numpy as np

from msf_check import ONE_BITS, SIGN, U64, key_of

OUT, IN, NEGATE, DROP_NONFINITE, REFUSE_NEGATIVE = 1, 2, 4, 8, 16
EXP = U64(0x7FF0000000000000)


class Refused(ValueError):
    def __init__(self, rid):
        super().__init__(f"relationship {rid} has a negative weight")
        self.id = rid


def weight_bits(rid, attr, flags, missing):
    """(bits after NEGATE and -0.0 -> +0.0, took `missing`)"""
    listed = rid in attr
    w = np.float64(attr[rid] if listed else missing)
    if listed and flags & NEGATE:
        w = -w
    b = np.array([w], dtype=np.float64).view(U64)[0]
    return (U64(0) if b == SIGN else b), not listed


def pair_weights(n, rels, attr, flags, active=None, missing=1.0):
    assert flags & (OUT | IN) and not flags & ~31
    rels = sorted(set((t, int(s), int(d), int(i)) for t, s, d, i in rels))
    rels = [r for r in rels if r[1] != r[2] and (active is None or (active[r[1]] and active[r[2]]))]
    per_pair = {}
    for t, s, d, _ in rels:
        per_pair[(t, s, d)] = per_pair.get((t, s, d), 0) + 1
    stats = [len(per_pair), len(rels), 0, 0, 0, 0, sum(1 for c in per_pair.values() if c > 1), 0]
    refused = []
    best, count = {}, {}
    for _, s, d, i in rels:
        b = ONE_BITS
        if attr is not None:
            b, took = weight_bits(i, attr, flags, missing)
            stats[5] += int(took)
            nonfinite = (b & EXP) == EXP
            if nonfinite and flags & DROP_NONFINITE:
                stats[4] += 1
                continue
            if not nonfinite and (b >> U64(63)) and flags & REFUSE_NEGATIVE:
                refused.append(i)
        cand = (int(key_of(b)[0]), i, int(b))
        for p in ([(s, d)] if flags & OUT else []) + ([(d, s)] if flags & IN else []):
            stats[2] += 1
            count[p] = count.get(p, 0) + 1
            if p not in best or cand < best[p]:
                best[p] = cand
    if refused:
        raise Refused(min(refused))
    keys = sorted(best)
    stats[3] = len(keys)
    stats[7] = max(count.values(), default=0)
    rows = np.array([k[0] for k in keys], dtype=U64)
    cols = np.array([k[1] for k in keys], dtype=U64)
    bits = None if attr is None else np.array([best[k][2] for k in keys], dtype=U64)
    kept = np.array([best[k][1] for k in keys], dtype=U64)
    return rows, cols, bits, kept, stats
