"""numpy restatement of the node-output dropout's mask function (csrc/gnm_dropout.hip, include/gnm.h), shared by
test_dropout_cpu.py (which checks it against the published Philox vectors) and test_gpu_dropout.py (which checks the kernels
against it bit for bit)."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Random123).  ctr: [..., 4] counter words, key: [..., 2] key words (any integer dtype, values < 2^32;
    broadcast against each other).  Returns the [..., 4] uint32 output."""
    ctr = np.asarray(ctr).astype(np.uint64)
    key = np.asarray(key).astype(np.uint64)
    c0, c1, c2, c3 = (ctr[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2             # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def keep_mask(node_ids, H, p, seed, step, layer):
    """bool [N,H]: element (row r, channel c) is kept.  node_ids: the caller's node id v of each row.  Counter (q_lo, q_hi, layer,
    step) with q = (v H + c) >> 2 in 64 bits, key (seed_lo, seed_hi); the draw is word c & 3; u = (x >> 8) 2^-24; kept iff
    u >= p in fp32."""
    v = np.asarray(node_ids).astype(np.uint64)[:, None]
    c = np.arange(H, dtype=np.uint64)[None, :]
    q = (v * np.uint64(H) + c) >> np.uint64(2)
    ctr = np.stack(np.broadcast_arrays(q & _LO, q >> _S32, np.uint64(layer), np.uint64(step)), -1)
    seed = int(seed) & (2 ** 64 - 1)
    out = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    x = np.take_along_axis(out, np.broadcast_to((c & np.uint64(3)).astype(np.int64), q.shape)[..., None], -1)[..., 0]
    u = (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def scale_of(p):
    """float(1 / (1 - p)), rounded once to fp32."""
    return np.float32(1.0 / (1.0 - float(p)))


def apply(x, keep, p):
    """where(mask, x * float32(1 / (1 - p)), +0) in fp32."""
    return np.where(keep, np.asarray(x, np.float32) * scale_of(p), np.float32(0.0)).astype(np.float32)
