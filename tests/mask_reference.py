"""numpy restatement of the read mask (include/gnm.h, gnm_read_mask; csrc/gnm_mask.hip) and of the thinned graph's degrees, shared
by test_mask_cpu.py (which checks the restatement's properties and the package's host route against it) and test_gpu_mask.py
(which checks the kernels against it bit for bit).  The Philox rounds are tests/dropout_reference.py's, which test_dropout_cpu.py
checks against the published vectors."""
import numpy as np

from dropout_reference import philox4x32_10

KEY_XOR = 0xA0761D6478BD642F            # GNM_READ_MASK_KEY_XOR
RANK_MIX = 0x9E3779B97F4A7C15           # engine.DROPOUT_RANK_MIX
_M64 = 2 ** 64 - 1


def mask_key(seed, rank=0):
    """(seed ^ rank * RANK_MIX) ^ KEY_XOR in 64 bits: engine.read_mask_key"""
    return ((int(seed) ^ (int(rank) * RANK_MIX)) ^ KEY_XOR) & _M64


def read_mask(n, f, key, epoch, graph_index):
    """bool [n]: node v is kept.  Read r = v >> 1, q = r >> 2; counter (q_lo, q_hi, graph_index, epoch), key (key_lo, key_hi);
    the draw is word r & 3; u = (x >> 8) 2^-24; kept iff u < f in fp32 (f rounded once from a double)."""
    v = np.arange(int(n), dtype=np.uint64)
    r = v >> np.uint64(1)
    q = r >> np.uint64(2)
    ctr = np.stack(np.broadcast_arrays(q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.uint64(int(graph_index) & 0xFFFFFFFF),
                                       np.uint64(int(epoch) & 0xFFFFFFFF)), -1)
    key = int(key) & _M64
    out = philox4x32_10(ctr, np.array([key & 0xFFFFFFFF, key >> 32], dtype=np.uint64)).reshape(-1, 4)
    x = out[np.arange(int(n)), (r & np.uint64(3)).astype(np.int64)]
    u = (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u < np.float32(float(f))


def degrees(src, dst, n):
    """(in-degree, out-degree) of an edge list as float32 [n] each: bincount"""
    return (np.bincount(np.asarray(dst, np.int64), minlength=n).astype(np.float32),
            np.bincount(np.asarray(src, np.int64), minlength=n).astype(np.float32))
