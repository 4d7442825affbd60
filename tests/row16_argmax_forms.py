"""Plain-Python restatement of the two forms of the 16-lane argmax of csrc/lane_ops.hpp (row16_argmax), lane by lane, with the DPP
exchange pattern the kernels use, and a numpy float32 restatement of csrc/sampler.hpp's draw for one head.  Test helper."""
import numpy as np

# partner lane of lane i in the four exchange steps: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
PARTNERS = ([i ^ 1 for i in range(16)], [i ^ 2 for i in range(16)], [(i & 8) | (7 - (i & 7)) for i in range(16)],
            [15 - i for i in range(16)])


def bits(x):
    """The float32 bit pattern as a signed 32-bit integer."""
    return int(np.float32(x).view(np.int32))


def exchange_argmax(values):
    """The four-step exchange: every lane carries (best, idx) and takes its partner's pair when that is lexicographically larger
    in (value, -index).  Returns the 16 lanes' (best, idx)."""
    best = [np.float32(v) for v in values]
    idx = list(range(16))
    for partner in PARTNERS:
        ob = [best[partner[i]] for i in range(16)]
        oi = [idx[partner[i]] for i in range(16)]
        for i in range(16):
            if (ob[i] > best[i]) or (ob[i] == best[i] and oi[i] < idx[i]):
                best[i], idx[i] = ob[i], oi[i]
    return best, idx


def _row_reduce(lanes, op):
    lanes = list(lanes)
    for partner in PARTNERS:
        lanes = [op(lanes[i], lanes[partner[i]]) for i in range(16)]
    return lanes


def max_then_lowest_index(values):
    """Row maximum of the bit patterns as signed integers, then row minimum of `bits == maximum ? lane : 16`.  Returns the 16
    lanes' (best, idx)."""
    b = [bits(v) for v in values]
    top = _row_reduce(b, max)
    idx = _row_reduce([i if b[i] == top[i] else 16 for i in range(16)], min)
    return [np.int32(t).view(np.float32) for t in top], idx


def sample_head(logits, q):
    """sample_row16 for one head in numpy float32: (action, logprob, entropy).  `logits` and `q` are the head's own columns."""
    f = np.float32
    logits, q = np.asarray(logits, f), np.asarray(q, f)
    mx = logits.max()
    ex = np.exp(logits - mx, dtype=f)
    se = ex.sum(dtype=f)
    with np.errstate(divide='ignore'):
        ratio = (ex / se) / q
    action = int(np.argmax(ratio))                      # first index among equals
    nl = logits - (mx + np.log(se, dtype=f))
    return action, float(nl[action]), float(-(nl * np.exp(nl, dtype=f)).sum(dtype=f))
