"""Host-side orchestration of the HIP kernels (libgnm.so) for the GatedGCN edge-logit path.

Everything here is plumbing: torch owns the memory and the stream, every arithmetic step is a
C-ABI call (include/gnm.h).  There is no torch / CPU fallback: tensors must live on a HIP
device and the library must load, otherwise the calls raise.

Layout: all [E,*] tensors inside the layer stack are in the graph's internal (destination
sorted) edge order; `model_forward` gathers e_raw into that order and scatters the scores
back to the caller's edge-id order.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import operator
import os
import threading
from dataclasses import dataclass, field, fields
from typing import Dict, List, Optional

import torch

from . import _lib

NT, NN, TN = 0, 1, 2
_D_FUSED = True    # Options.FUSED: use the W-stationary fused MFMA kernels where they exist (H = 128); tests flip it
EPS_BN = 1e-5   # nn.BatchNorm1d default (gated_gcn_full.py:55-56)

LIN5 = ("A_1", "A_2", "A_3", "B_1", "B_2")

# What a training forward keeps for the backward pass:
#   "saved"  every intermediate the backward kernels read: per layer P [N,5H], t [E,H], e_out [E,H], hf, inv_f, hb,
#            inv_b, z [N,H] (137 GiB at N=1.5 M / E=7.54 M / H=128 / L=8);
#   "lean"   P and t are NOT kept: the backward of a layer first re-runs the two kernels that produced them
#            (node projections, then the fused edge-t kernel) from h_in / e_in, which ARE kept (e_in is the previous
#            layer's e_out).  Bit-identical results (same kernels, same inputs), about 7 GiB less per layer at the
#            size above, for two extra kernels per layer (+3.3 ms of 25).
# Independent of the mode: model_forward(checkpoint=k) keeps of the layer stack only the inputs of every k-th layer and model_backward
# recomputes one k-layer segment at a time (checkpoint_segments; a property of the call kept in ModelSaved, not an Options switch).
_D_ACTIVATIONS = os.environ.get("GNM_ACTIVATIONS", "saved").strip().lower()


_OPTION_NAMES = ("FUSED", "ACTIVATIONS", "CHAIN", "TN_SIDE", "TN_SIDE_CAP", "SRC_SIDE_CAP", "TN_AT", "TN_SPLIT", "TWO_SIDED", "TWO_SIDED_FWD", "WIDE_FUSED",
                 "NODE_FUSED", "LN_SWEEP")


class Options:
    """The schedule switches of a pass (FUSED, ACTIVATIONS, CHAIN, TN_SIDE, TN_SIDE_CAP, SRC_SIDE_CAP, TN_AT, TN_SPLIT, TWO_SIDED,
    TWO_SIDED_FWD, WIDE_FUSED, NODE_FUSED, LN_SWEEP; what each selects is described where its default is defined below) as ONE immutable
    object.  They choose between schedules that compute the same thing (tests and bench.py A/B them).  model_forward /
    layer_forward read the object that is current in the calling thread -- `current()`: the innermost `with options(...)` /
    `with use(opts)` of THIS thread, else the process defaults (environment, `set_default`) -- and the autograd functions of
    models.py / layers.py keep it with the saved activations, so that the backward of a forward runs under the SAME switches
    whatever thread autograd runs it on and whatever the caller has changed since."""
    __slots__ = _OPTION_NAMES

    def __init__(self, **kw):
        for k in _OPTION_NAMES:
            object.__setattr__(self, k, kw[k])

    def __setattr__(self, k, v):
        raise AttributeError("engine.Options is immutable: use replace(), options(...) or set_default(...)")

    def replace(self, **kw) -> "Options":
        bad = [k for k in kw if k not in _OPTION_NAMES]
        if bad:
            raise _lib.GnmError(f"engine.options: unknown switch {bad}; known: {_OPTION_NAMES}")
        if "ACTIVATIONS" in kw and kw["ACTIVATIONS"] not in ("saved", "lean"):
            raise _lib.GnmError(f"activation mode {kw['ACTIVATIONS']!r}: expected 'saved' or 'lean'")
        if "TN_AT" in kw and kw["TN_AT"] not in ("now", "next", "auto"):
            raise _lib.GnmError(f"TN_AT {kw['TN_AT']!r}: expected 'now', 'next' or 'auto'")
        d = {k: getattr(self, k) for k in _OPTION_NAMES}
        d.update(kw)
        return Options(**d)

    def __repr__(self):
        return "Options(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in _OPTION_NAMES) + ")"


_tls = threading.local()
_default: Optional[Options] = None          # built from the _D_* definitions at the end of this module


def current() -> Options:
    """The options of the calling thread (see Options)."""
    o = getattr(_tls, "opts", None)
    return o if o is not None else _default


@contextlib.contextmanager
def use(opts: Optional[Options]):
    """Run the body under `opts` in this thread (None: leave things as they are)."""
    if opts is None:
        yield current()
        return
    prev = getattr(_tls, "opts", None)
    _tls.opts = opts
    try:
        yield opts
    finally:
        _tls.opts = prev


@contextlib.contextmanager
def options(**kw):
    """`with engine.options(TWO_SIDED=False, CHAIN=False): ...` -- the current options of this thread with some switches
    changed, for the body; restored on exit whatever happens inside.  Thread-local: another thread never sees them."""
    with use(current().replace(**kw)) as o:
        yield o


def set_default(**kw) -> None:
    """Change the process-wide defaults (what a thread outside any options() / use() block runs under): start-up configuration."""
    global _default
    _default = _default.replace(**kw)


def _scoped(saved_arg: Optional[int] = None):
    """Give a pass an `opts=` keyword: the Options it runs under.  A backward pass without one runs under the options its
    forward left in the saved state (positional argument `saved_arg`)."""
    def deco(fn):
        @functools.wraps(fn)
        def w(*a, opts: Optional[Options] = None, **k):
            if opts is None and saved_arg is not None and len(a) > saved_arg:
                opts = getattr(a[saved_arg], "opts", None)
                scoped = getattr(_tls, "opts", None)
                if scoped is not None and getattr(a[saved_arg], "dropout", None) is not None:
                    scoped = _dropout_opts(scoped)      # what a forward with dropout saves of them: no difference to warn about
                if opts is not None and scoped is not None and scoped is not opts and repr(scoped) != repr(opts):
                    # `with engine.options(...)` around a backward only: the saved forward options win (the backward kernels must
                    # match the activations the forward kept) -- say so instead of silently comparing two identical paths
                    import warnings
                    warnings.warn("engine: this backward runs under the options its forward saved "
                                  f"({opts!r}); the options scoped around the backward call ({scoped!r}) are ignored -- scope the "
                                  "forward, or pass opts= explicitly", stacklevel=2)
            if opts is None:
                return fn(*a, **k)
            with use(opts):
                return fn(*a, **k)
        return w
    return deco


def __getattr__(name):          # engine.CHAIN, engine.ACTIVATIONS, ...: the current value (read-only; PEP 562)
    if name in _OPTION_NAMES:
        return getattr(current(), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def set_activation_mode(mode: str) -> None:
    """Process-wide default of Options.ACTIVATIONS ('saved' / 'lean')."""
    set_default(ACTIVATIONS=mode)



def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_device_of(pick):
    """Run the wrapped entry point with the HIP device of `pick(*args)` current.  HIP launches go to the CURRENT
    device and _stream() is the current device's stream; the reference's own pattern is model.to('cuda:3') with
    no set_device (hyperparameters.py:25), so without this the kernels would be queued on device 0 with
    device-3 pointers."""
    def deco(fn):
        @functools.wraps(fn)
        def wrapper(*a, **k):
            t = pick(*a, **k)
            dev = t.device if torch.is_tensor(t) else torch.device(t)
            if dev.type != "cuda":
                raise _lib.GnmError("gnnome_assembly_amd: tensors must be on a HIP device (no CPU fallback)")
            if dev.index is None or dev.index == torch.cuda.current_device():
                return fn(*a, **k)
            with torch.cuda.device(dev):
                return fn(*a, **k)
        return wrapper
    return deco


# Optional per-op timing (bench.py / profiling only): when `_prof` is a list every C-ABI call is
# bracketed by HIP events recorded on the stream the kernels are launched on.
_prof = None


def profile_ops(enable: bool):
    """Start (True) or stop (False) per-op event timing; stop returns {op: (calls, total_ms)}."""
    global _prof
    if enable:
        _prof = []
        return None
    rec, _prof = _prof, None
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1 in rec or []:
        c, t = out.get(name, (0, 0.0))
        out[name] = (c + 1, t + e0.elapsed_time(e1))
    return out


def _call(name: str, *args, tag: str = None):
    fn = getattr(_lib.load(), name)
    if _prof is None:
        rc = fn(*args)
    else:
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        _prof.append((tag or name, e0, e1))
    _lib.check(rc, name)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _chk_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.GnmError("gnnome_assembly_amd: tensors must be on a HIP device (no CPU fallback)")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise _lib.GnmError(f"expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


# The argument rules of the wrappers from bce_with_logits down: each of these raises or returns, and a wrapper states what it
# requires of every argument by calling them before its first launch.
def _fits(t: torch.Tensor, dt, m: int) -> bool:
    return t.dtype == dt and t.numel() == m and t.is_contiguous()


def _chk_args(fn: str, *rows, optional=()):
    """Every row (name, tensor, dtype, elements) of wrapper `fn` is a contiguous tensor of that dtype and size; the names in
    `optional` may be None."""
    for name, t, dt, m in rows:
        if not (t is None and name in optional) and not _fits(t, dt, m):
            raise ValueError(f"{fn}: {name} must be a contiguous {str(dt).replace('torch.', '')} [{m}] tensor")


def _chk_record(fn: str, rec, words: int, name: str = "record", owner: str = ""):
    """`rec` holds a device record of `words` int64 words; `owner`: the object whose buffer it usually is, for the message."""
    if not _fits(rec, torch.int64, words):
        raise ValueError(f"{fn}: {name} must be a contiguous int64 [{words}] tensor{owner}")


def _chk_epoch_acc(scores, epoch_acc):
    if epoch_acc is not None:
        _chk_dev(scores, epoch_acc)
        if not _fits(epoch_acc, torch.int64, 6):
            raise ValueError("epoch_acc: a contiguous int64 [6] tensor (train.EpochStats.buf)")


def _chk_index(fn: str, idx, keys, n: int):
    """The arrays `keys` of a graph index, and its node permutation [n] when it has one, are contiguous int32 tensors."""
    nperm = idx.get("nperm")
    if any(idx[k].dtype != torch.int32 or not idx[k].is_contiguous() for k in keys) or \
            (nperm is not None and not _fits(nperm, torch.int32, n)):
        raise ValueError(f"{fn}: the index arrays must be contiguous int32 tensors (graph.index())")


def _scores_labels(fn: str, scores, y):
    """(scores, labels or None, E) as flat contiguous fp32 tensors of E entries each."""
    x = _f32c(scores.detach().reshape(-1).float())     # .float(): a half or bf16 tensor is compared as its fp32 copy (exact widening)
    E = x.numel()
    if y is not None:
        y = _f32c(y.reshape(-1).float())
        if y.numel() != E:
            raise ValueError(f"{fn}: {E} scores, {y.numel()} labels")
    return x, y, E


class _Scratch:
    """Per-device scratch buffers (torch-owned; the library never allocates)."""

    def __init__(self, device):
        lib = _lib.load()
        self.device = device
        self.max_blocks = lib.gnm_max_partial_blocks()
        # (max_blocks + 1) rows: the extra row is the reduction scratch of gnm_bn_*finalize (gnm.h)
        self.partials = torch.empty((self.max_blocks + 1) * 2 * 256, dtype=torch.float64, device=device)
        self._ws = torch.empty(1 << 20, dtype=torch.uint8, device=device)

    def ws(self, nbytes: int) -> torch.Tensor:
        if self._ws.numel() < nbytes:
            self._ws = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=self.device)
        return self._ws


_scratch: Dict[tuple, _Scratch] = {}


def scratch(device, key: str = "main") -> _Scratch:
    device = torch.device(device)
    if (device, key) not in _scratch:
        _scratch[(device, key)] = _Scratch(device)
    return _scratch[(device, key)]


_side_streams: Dict[torch.device, "torch.cuda.Stream"] = {}


def _side_stream(device):
    device = torch.device(device)
    if device not in _side_streams:
        _side_streams[device] = torch.cuda.Stream(device=device)
    return _side_streams[device]


class SideLane:
    """The side stream of ONE backward pass (model_backward makes it and drains it): weight gradients with no consumer before
    the optimizer step run there, beside HBM-bound passes of the main stream (see TN_SIDE).  The schedules decide WHEN to
    launch; the lane knows HOW.  It keeps what the side stream reads alive until the main stream has waited for it (no
    record_stream: blocks parked on a side-stream event made the allocator fall back to hipMalloc / hipFree in the lean mode:
    3x the step time), and its scratch is allocated and grown only with the side stream current, so a block it gives up goes
    back to the side stream's pool.  Main-stream launches never use that scratch."""

    def __init__(self, device):
        self.device = device
        self.side = _side_stream(device)
        self.main = torch.cuda.current_stream(device)
        self.held: List[torch.Tensor] = []
        self.sc: Optional[_Scratch] = None      # made at the first launch

    def begin(self) -> None:
        """Ready for one more launch: the main stream first waits for what ran there before (a layer ago: free) -- which also
        makes the held tensors safe to drop -- and the side stream for the main stream's work so far."""
        self.main.wait_stream(self.side)
        self.held.clear()
        self.side.wait_stream(self.main)

    def wait_for_main(self) -> None:
        """A further launch since begin(): the side stream only waits for the main stream's work so far."""
        self.side.wait_stream(self.main)

    def drain(self) -> None:
        """The main stream waits for everything launched here; the held tensors are released."""
        self.main.wait_stream(self.side)
        self.held.clear()

    def _ws(self, need: int) -> torch.Tensor:
        with torch.cuda.stream(self.side):
            self.sc = self.sc or scratch(self.device, "side")
            return self.sc.ws(need)

    def node_proj_bwd_tn(self, N: int, H: int, gP, h, W, b) -> None:
        lib = _lib.load()
        need = lib.gnm_node_proj_bwd_workspace_bytes(5 * H)
        ws = self._ws(need)
        _lib.check(lib.gnm_node_proj_bwd_tn(N, H, 5 * H, _ptr(gP), _ptr(h), _ptr(W), _ptr(b), _ptr(self.sc.partials), _ptr(ws), need,
                                            current().TN_SIDE_CAP, C.c_void_p(self.side.cuda_stream)), "gnm_node_proj_bwd_tn")
        self.held += (gP, h, W, b)

    def tn128(self, N: int, A, lda: int, ncg: int, h, W, b) -> None:
        lib = _lib.load()
        need = lib.gnm_tn128_workspace_bytes()
        ws = self._ws(need)
        _lib.check(lib.gnm_tn128(N, _ptr(A), lda, ncg, _ptr(h), _ptr(W), _ptr(b), _ptr(self.sc.partials), _ptr(ws), need,
                                 C.c_void_p(self.side.cuda_stream)), "gnm_tn128")
        self.held += (A, h, W, b)

    def gemm_tn_colsum(self, A, B, C_, out) -> None:
        """gemm_tn_colsum(A, B, C_, out) here (the shapes are the layer's own)."""
        lib = _lib.load()
        (K, M), N = A.shape, B.shape[1]
        need = lib.gnm_gemm_tn_colsum_workspace_bytes(M, N, K)
        ws = self._ws(need) if need else None
        _lib.check(lib.gnm_gemm_tn_colsum(M, N, K, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(C_), C_.stride(0), _ptr(out),
                                          _ptr(ws), need, C.c_void_p(self.side.cuda_stream)), "gnm_gemm_tn_colsum")
        self.held += (A, B, C_, out)


# ---------------------------------------------------------------------------------------
# thin wrappers
# ---------------------------------------------------------------------------------------

@on_device_of(lambda mode, A, *a, **k: A)
def gemm(mode: int, A: torch.Tensor, B: torch.Tensor, C_: torch.Tensor, bias=None, resid=None, relu=False):
    """C = op(A) op(B) (+bias +resid, relu).  A, B, C, resid are 2-D views with unit inner
    stride; shapes follow include/gnm.h (NT: A[M,K] B[N,K]; NN: A[M,K] B[K,N]; TN: A[K,M] B[K,N])."""
    lib = _lib.load()
    _chk_dev(A, B, C_, bias, resid)
    for t in (A, B, C_, resid):
        if t is not None and (t.dim() != 2 or t.stride(1) != 1 or t.dtype != torch.float32):
            raise _lib.GnmError("gemm: operands must be 2-D float32 with unit inner stride")
    if mode == NT:
        M, K = A.shape
        N, K2 = B.shape
    elif mode == NN:
        M, K = A.shape
        K2, N = B.shape
    else:
        K, M = A.shape
        K2, N = B.shape
    if K != K2 or tuple(C_.shape) != (M, N):
        raise _lib.GnmError(f"gemm: shape mismatch mode={mode} A={tuple(A.shape)} B={tuple(B.shape)} C={tuple(C_.shape)}")
    need = lib.gnm_gemm_f32_workspace_bytes(mode, M, N, K)
    ws = scratch(A.device).ws(need) if need else None
    _call("gnm_gemm_f32", mode, M, N, K, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(C_),
                                C_.stride(0), _ptr(bias), _ptr(resid),
                                resid.stride(0) if resid is not None else 0, int(bool(relu)),
                                _ptr(ws), need, _stream(),
          tag=f"gemm_{('NT', 'NN', 'TN')[mode]}[{M}x{N}x{K}]" if _prof is not None else None)
    return C_


@on_device_of(lambda A, *a, **k: A)
def gemm_tn_colsum(A: torch.Tensor, B: torch.Tensor, C_: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C = A^T B and the column sums of A (weight and bias gradient of a Linear: A = grad of its output [rows, out],
    B = its input [rows, in]); returns the column sums."""
    lib = _lib.load()
    _chk_dev(A, B, C_, out)
    for t in (A, B, C_):
        if t.dim() != 2 or t.stride(1) != 1 or t.dtype != torch.float32:
            raise _lib.GnmError("gemm_tn_colsum: operands must be 2-D float32 with unit inner stride")
    K, M = A.shape
    K2, N = B.shape
    if K != K2 or tuple(C_.shape) != (M, N):
        raise _lib.GnmError(f"gemm_tn_colsum: shape mismatch A={tuple(A.shape)} B={tuple(B.shape)} C={tuple(C_.shape)}")
    if out is None:
        out = torch.empty(M, dtype=torch.float32, device=A.device)
    need = lib.gnm_gemm_tn_colsum_workspace_bytes(M, N, K)
    ws = scratch(A.device).ws(need) if need else None
    _call("gnm_gemm_tn_colsum", M, N, K, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(C_), C_.stride(0), _ptr(out),
          _ptr(ws), need, _stream(), tag=f"gemm_TN+colsum[{M}x{N}x{K}]" if _prof is not None else None)
    return out


@on_device_of(lambda X, *a, **k: X)
def colsum(X: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    _chk_dev(X)
    M, W = X.shape
    if out is None:
        out = torch.empty(W, dtype=torch.float32, device=X.device)
    need = lib.gnm_colsum_workspace_bytes(M, W)
    ws = scratch(X.device).ws(need)
    _call("gnm_colsum_f32", M, W, _ptr(X), X.stride(0), _ptr(out), _ptr(ws), need, _stream())
    return out


def bn_finalize(partials, nblk, count, H, gamma, beta):
    lib = _lib.load()
    stat = torch.empty(4, H, dtype=torch.float32, device=gamma.device)
    _call("gnm_bn_finalize", _ptr(partials), nblk, count, H, _ptr(gamma), _ptr(beta), EPS_BN,
                                   _ptr(stat), _stream())
    return stat


def bn_bwd_finalize(partials, nblk, count, H, device, gg=None, gb=None):
    lib = _lib.load()
    bstat = torch.empty(2, H, dtype=torch.float32, device=device)
    gg = torch.empty(H, dtype=torch.float32, device=device) if gg is None else gg
    gb = torch.empty(H, dtype=torch.float32, device=device) if gb is None else gb
    _call("gnm_bn_bwd_finalize", _ptr(partials), nblk, count, H, _ptr(bstat), _ptr(gg), _ptr(gb),
                                       _stream())
    return bstat, gg, gb


def node_rows_in(idx, x: torch.Tensor) -> torch.Tensor:
    """[N,W] rows in the caller's node numbering -> the graph's internal numbering (a gather through idx['nperm'];
    the tensor itself when the index keeps the caller's numbering)."""
    nperm = idx.get("nperm")
    if nperm is None:
        return x
    out = torch.empty_like(x)
    _call("gnm_gather_rows_f32", x.shape[0], x.shape[1], _ptr(x), _ptr(nperm), _ptr(out), _stream())
    return out


def edge_rank(idx) -> torch.Tensor:
    """The inverse of idx['perm']: internal position of each caller edge id (int32 [E], built once per index and kept in
    it).  A gather through it takes [E,W] rows from the internal order back to the caller's edge-id order."""
    er = idx.get("erank")
    if er is None:
        perm = idx["perm"]
        er = torch.empty_like(perm)
        er[perm.long()] = torch.arange(perm.numel(), dtype=perm.dtype, device=perm.device)
        idx["erank"] = er
    return er


def node_rows_out(idx, x: torch.Tensor) -> torch.Tensor:
    """The inverse of node_rows_in: internal numbering -> the caller's."""
    nrank = idx.get("nrank")
    if nrank is None:
        return x
    out = torch.empty_like(x)
    _call("gnm_gather_rows_f32", x.shape[0], x.shape[1], _ptr(x), _ptr(nrank), _ptr(out), _stream())
    return out


# ---------------------------------------------------------------------------------------
# node-output dropout of the layer stack (gated_gcn_full.py:154): counter-based masks, nothing stored (gnm_dropout.hip)
# ---------------------------------------------------------------------------------------
# A pass takes dropout=(p, key, step): the keep decision of (layer, caller's node id, channel) is a pure function of those, so the
# backward, a checkpoint recomputation and a test all re-derive the mask the forward used.  p = 0 / None: no launch, nothing changes.
_M64 = (1 << 64) - 1
DROPOUT_RANK_MIX = 0x9E3779B97F4A7C15       # the key of data-parallel rank r is seed ^ r * this (mod 2^64)
_dropout_state: Dict[torch.device, list] = {}       # device -> [seed, step]: the stream the MODULES draw (key, step) from


def dropout_p(p) -> float:
    """A module's dropout argument as a float in [0, 1), or ValueError (what GatedGCN_1d raises)."""
    try:
        ok = 0 <= p < 1
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"dropout={p!r}: expected a probability 0 <= p < 1")
    return float(p)


def dropout_key(seed: int, rank: Optional[int] = None) -> int:
    """The 64-bit Philox key of a data-parallel rank: seed ^ rank * 0x9E3779B97F4A7C15 (rank None: this process's, dp.current_rank)."""
    if rank is None:
        from . import dp
        rank = dp.current_rank()
    return (int(seed) ^ (int(rank) * DROPOUT_RANK_MIX)) & _M64


def _dropout_dev(device) -> torch.device:
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if device.type == "cuda" and device.index is None else device


def dropout_seed(seed: int, step: int = 0, device=None) -> None:
    """Set the seed of `device`'s dropout stream (default: the current device) and restart its step counter at `step`: the
    forwards that follow draw the masks they drew after the same call before.  Without a call the seed is torch.initial_seed()
    at the first training forward with p > 0."""
    _dropout_state[_dropout_dev(device)] = [int(seed) & _M64, int(step) & 0xFFFFFFFF]


def dropout_draw(p: float, device=None):
    """(p, key, step) for ONE training forward with p > 0 on `device`: the key of this rank, the step counter's value, which
    is then incremented (32 bits, wrapping)."""
    st = _dropout_state.setdefault(_dropout_dev(device), [torch.initial_seed() & _M64, 0])
    step = st[1]
    st[1] = (step + 1) & 0xFFFFFFFF
    return (float(p), dropout_key(st[0]), step)


def _dropout_arg(dropout):
    """A pass's `dropout` argument as (p, key, step) with p > 0, or None (no dropout)."""
    if dropout is None:
        return None
    p, key, step = dropout
    p = dropout_p(p)
    return (p, int(key) & _M64, int(step) & 0xFFFFFFFF) if p > 0 else None


@on_device_of(lambda x, *a, **k: x)
def node_dropout(x: torch.Tensor, dropout, layer: int, width: Optional[int] = None, node_ids: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mask * x / (1 - p) of layer `layer`'s node rows x [N, ld] (gnm_node_dropout_apply), IN PLACE unless `out` (same shape) is
    given.  width: the model's real width when x is zero-padded to a kernel width (columns width .. ld-1 are left alone).
    node_ids: caller's node id of each row (int32 [N]: the index's 'nperm'); None: the row number.  Its own backward."""
    drop = _dropout_arg(dropout)
    y = x if out is None else out
    _chk_dev(x, y, node_ids)
    if (x.dim() != 2 or x.stride(1) != 1 or x.dtype != torch.float32 or y.shape != x.shape or y.dtype != x.dtype
            or y.stride() != x.stride()):
        raise _lib.GnmError("node_dropout: x (and out) must be 2-D float32 with unit inner stride and the same layout")
    if node_ids is not None and (node_ids.dtype != torch.int32 or node_ids.numel() != x.shape[0] or not node_ids.is_contiguous()):
        raise _lib.GnmError("node_dropout: node_ids must be a contiguous int32 [N] tensor")
    if drop is None:
        return y if out is None else y.copy_(x)
    H = x.shape[1] if width is None else int(width)
    _call("gnm_node_dropout_apply", x.shape[0], H, x.stride(0), _ptr(x), _ptr(y), _ptr(node_ids), drop[0], drop[1], drop[2], int(layer),
          _stream())
    return y


def dropout_mask(N: int, H: int, dropout, layer: int, device, node_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The keep decisions node_dropout takes, as a uint8 [N,H] tensor (gnm_node_dropout_mask).  node_ids None: row v is the
    caller's node v -- the mask of a model's layer in the caller's numbering, whatever the graph's internal order."""
    drop = _dropout_arg(dropout)
    if drop is None:
        raise _lib.GnmError("dropout_mask: p = 0 has no mask")
    _chk_dev(node_ids)
    if node_ids is not None and (node_ids.dtype != torch.int32 or node_ids.numel() != N or not node_ids.is_contiguous()):
        raise _lib.GnmError("dropout_mask: node_ids must be a contiguous int32 [N] tensor")
    with torch.cuda.device(device):
        mask = torch.empty(N, H, dtype=torch.uint8, device=device)
        _call("gnm_node_dropout_mask", N, H, _ptr(mask), _ptr(node_ids), drop[0], drop[1], drop[2], int(layer), _stream())
    return mask


def _dropout_opts(o: "Options") -> "Options":
    """The switches a pass with p > 0 runs under: the gradient entering a layer's node backward must exist as a finished [N,H]
    tensor, so the one schedule that consumes it inside a matrix kernel's epilogue is pinned off -- NODE_FUSED (the projection
    backward that also takes the BatchNorm_h backward sums of the layer below: gnm_node_proj_bwd_nn_stats)."""
    return o.replace(NODE_FUSED=False) if o.NODE_FUSED else o


# ---------------------------------------------------------------------------------------
# read-masking coverage augmentation (gnm_mask.hip): the mask of a training step, the degrees of the thinned graph
# ---------------------------------------------------------------------------------------
READ_MASK_KEY_XOR = 0xA0761D6478BD642F      # GNM_READ_MASK_KEY_XOR of include/gnm.h: odd, so the key never equals the dropout key


def read_mask_key(seed: int, rank: Optional[int] = None) -> int:
    """The Philox key of a rank's read masks: dropout_key(seed, rank) ^ READ_MASK_KEY_XOR -- the rank-mixed key of the dropout
    stream moved by a fixed constant, so that the two streams of one seed never share a (key, counter) pair."""
    return (dropout_key(seed, rank) ^ READ_MASK_KEY_XOR) & _M64


def read_mask_fraction(f) -> float:
    """A kept fraction as a float in [0, 1], or ValueError."""
    try:
        ok = 0 <= f <= 1
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"read mask fraction {f!r}: expected 0 <= f <= 1")
    return float(f)


def read_mask(n: int, f: float, key: int, epoch: int, graph_index: int, device, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bool [n]: node v (the caller's numbering; nodes 2i, 2i+1 are the strands of read i) is kept (gnm_read_mask, one launch on
    the current stream of `device`).  A pure function of (f, key, epoch, graph_index, v).  `out`: a contiguous uint8 [n] tensor
    to fill (any alignment); the result is its bool view."""
    f = read_mask_fraction(f)
    device = _dropout_dev(device)
    if device.type != "cuda":
        raise _lib.GnmError("read_mask: needs a HIP device (cluster.masked_subgraph has the host route for graphs on the CPU)")
    n = int(n)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(max(n, 0), dtype=torch.uint8, device=device)
        elif out.dtype != torch.uint8 or out.numel() != n or not out.is_contiguous() or out.device != device:
            raise _lib.GnmError("read_mask: out must be a contiguous uint8 [n] tensor on the device")
        _call("gnm_read_mask", n, f, int(key) & _M64, int(epoch) & 0xFFFFFFFF, int(graph_index) & 0xFFFFFFFF, _ptr(out), _stream())
    return out.view(torch.bool)


@on_device_of(lambda idx, pe: pe)
def index_degrees(idx, pe: torch.Tensor) -> torch.Tensor:
    """Columns 0 and 1 of pe [n, ld] (fp32, the caller's node order, written IN PLACE) = the in- and out-degrees the index `idx`
    (dict of graph.index()) holds: gnm_index_degrees, one launch.  The other columns are left alone."""
    n = int(idx["in_ptr"].numel()) - 1
    nperm = idx.get("nperm")
    _chk_dev(pe, idx["in_ptr"], idx["out_ptr"], nperm)
    if pe.dim() != 2 or pe.dtype != torch.float32 or pe.shape[0] != n or pe.shape[1] < 2 or (n > 0 and pe.stride(1) != 1):
        raise _lib.GnmError("index_degrees: pe must be a float32 [n, >= 2] tensor with unit inner stride, n the index's node count")
    _call("gnm_index_degrees", n, _ptr(idx["in_ptr"]), _ptr(idx["out_ptr"]), _ptr(nperm), _ptr(pe), pe.stride(0) if n > 0 else pe.shape[1],
          _stream())
    return pe


# ---------------------------------------------------------------------------------------
# one GatedGCN layer
# ---------------------------------------------------------------------------------------

@dataclass
class LayerParams:
    """Views of one GatedGCN_1d's parameters (gated_gcn_full.py:44-59)."""
    W5: torch.Tensor       # [5H,H] = cat(A_1,A_2,A_3,B_1,B_2).weight
    b5: torch.Tensor       # [5H]
    W3: torch.Tensor       # B_3.weight [H,H]
    b3: torch.Tensor
    gamma_e: torch.Tensor
    beta_e: torch.Tensor
    gamma_h: torch.Tensor
    beta_h: torch.Tensor


@dataclass
class LayerSaved:
    h_in: torch.Tensor = None
    e_in: torch.Tensor = None
    P: torch.Tensor = None
    t: torch.Tensor = None
    stat_e: torch.Tensor = None
    e_out: torch.Tensor = None
    hf: torch.Tensor = None
    inv_f: torch.Tensor = None
    hb: torch.Tensor = None
    inv_b: torch.Tensor = None
    z: torch.Tensor = None
    stat_h: torch.Tensor = None
    opts: "Options" = None       # the switches the forward ran under: its backward runs under the same (see Options)
    chunks: list = None          # a layer wider than 256: the saved state of its 256-column problems (see WIDE_CHUNK)
    matmul: str = None           # the matmul mode (process-wide, not an Option) the forward ran in: its backward must run in the same


def _proj_and_t(idx, N, E, H, prm, h_in, e_in, nblk):
    """P = h W5^T + b5 [N,5H] and t = e W3^T + b3 + B1h[src] + B2h[dst] [E,H] (gated_gcn_full.py:107-113,120-121);
    leaves the BatchNorm partial sums of t in the scratch buffer and their count in nblk.  H is the layer's OUTPUT
    width; h_in / e_in may be narrower or wider (in_channels != out_channels: the generic GEMM route)."""
    lib = _lib.load()
    dev = h_in.device
    sc = scratch(dev)
    st = _stream()
    P = torch.empty(N, 5 * H, dtype=torch.float32, device=dev)
    t = torch.empty(E, H, dtype=torch.float32, device=dev)
    if H == 128 and current().FUSED and h_in.shape[1] == H:
        # W-stationary fused MFMA path: projections, then t + BatchNorm partials in one pass
        need = lib.gnm_rowtile_workspace_bytes(5 * H)
        ws = sc.ws(need)
        _call("gnm_node_proj_fwd", N, H, 5 * H, _ptr(h_in), _ptr(prm.W5), _ptr(prm.b5), _ptr(P), _ptr(ws), need, st)
        _call("gnm_edge_t_fused_fwd", E, H, _ptr(e_in), _ptr(prm.W3), _ptr(prm.b3), _ptr(P), _ptr(idx["isrc"]),
              _ptr(idx["idst"]), _ptr(t), _ptr(sc.partials), C.byref(nblk), _ptr(ws), need, st)
    elif H == 256 and current().FUSED and current().WIDE_FUSED and e_in.shape[1] == H and _lib.split_mode():
        # the reference's default width: projections through the split-mode GEMM, t + BatchNorm partials in one pass
        # (a workgroup keeps one 128-column half of W3 stationary in eight waves)
        gemm(NT, h_in, prm.W5, P, bias=prm.b5)
        need = lib.gnm_rowtile_workspace_bytes(5 * H)
        ws = sc.ws(need)
        _call("gnm_edge_t_fused_fwd", E, H, _ptr(e_in), _ptr(prm.W3), _ptr(prm.b3), _ptr(P), _ptr(idx["isrc"]),
              _ptr(idx["idst"]), _ptr(t), _ptr(sc.partials), C.byref(nblk), _ptr(ws), need, st, tag="gnm_edge_t_fused_fwd[256]")
    else:
        # dense projections                                                    (:107-113)
        gemm(NT, h_in, prm.W5, P, bias=prm.b5)
        gemm(NT, e_in, prm.W3, t, bias=prm.b3)
        # t += B1h[src] + B2h[dst], BatchNorm statistics over all E edges       (:120-122)
        _call("gnm_edge_t_stats_fwd", E, H, _ptr(t), _ptr(P), _ptr(idx["isrc"]), _ptr(idx["idst"]),
              _ptr(sc.partials), C.byref(nblk), st)
    return P, t


@on_device_of(lambda idx, N, E, H, prm, h_in, *a, **k: h_in)
@_scoped()
def layer_forward(idx, N: int, E: int, H: int, prm: LayerParams, h_in, e_in, save: bool, batch_norm: bool = True,
                  residual: bool = True, plan: Optional[dict] = None, ln_width: Optional[int] = None, wide_ln: Optional[bool] = None):
    """GatedGCN_1d.forward (gated_gcn_full.py:99-157) on internal-order tensors.
    Returns (h_out, e_out, LayerSaved or None).  H = out_channels; h_in [N,Hin], e_in [E,Hin] with Hin != H only
    when residual is False (the reference drops the residual then: gated_gcn_full.py:41-42).
    plan (graph.sweep_plan(device, 2), BatchNorm, H = 128 or 256): gate + by-source aggregation as ONE two-sided sweep.
    ln_width (LayerNorm mode, a layer zero-padded to the kernel width H): the layer's real out_channels -- nn.LayerNorm
    normalises over those (gated_gcn_full.py:58-59), the dead channels are left out of the row statistics.
    wide_ln (LayerNorm mode, H > 256): the opt-in a GatedGCN_1d recorded at construction (layers.WIDE_LAYERNORM); None: the
    switch's current value.  Off, such a layer raises NotImplementedError as before."""
    lnw = H if ln_width is None else int(ln_width)
    if residual and h_in.shape[1] != H:
        raise _lib.GnmError("layer_forward: a residual layer needs in_channels == out_channels")
    if H > WIDE_CHUNK:
        return _wide_layer_forward(idx, N, E, H, prm, h_in, e_in, save, batch_norm, residual, plan, lnw, wide_ln)
    nblk = C.c_int(0)
    P, t = _proj_and_t(idx, N, E, H, prm, h_in, e_in, nblk)
    return _layer_forward_tail(idx, N, E, H, prm, h_in, e_in, P, t, nblk, save, batch_norm, residual, plan, lnw)


def _layer_forward_tail(idx, N, E, H, prm, h_in, e_in, P, t, nblk, save, batch_norm, residual, plan, lnw):
    """layer_forward behind the two dense products: everything from the gate to h_out.  With BatchNorm this part is separable by
    COLUMNS (per-channel statistics, per-channel gates): a layer wider than the kernels runs it once per 256-column chunk."""
    res_e = _ptr(e_in) if residual else C.c_void_p(0)
    res_h = _ptr(h_in) if residual else C.c_void_p(0)
    lib = _lib.load()
    dev = h_in.device
    sc = scratch(dev)
    st = _stream()
    f32 = dict(dtype=torch.float32, device=dev)
    # gate, edge output, by-destination gated mean                         (:122-130)
    e_out = torch.empty(E, H, **f32)
    hf = torch.empty(N, H, **f32)
    # 256: one sweep per 128-column half (BatchNorm); LayerNorm: H = 128 (row statistics inside the sweep, no barrier)
    two_sided = plan is not None and (H in (128, 256) if batch_norm else H == 128) and current().TWO_SIDED_FWD
    inv_f = torch.empty(N, H, **f32) if (save or not two_sided) else None      # inv_f / inv_b: only the backward reads them
    if two_sided and not batch_norm:
        hb = torch.empty(N, H, **f32)
        inv_b = torch.empty(N, H, **f32) if save else None
        z = torch.empty(N, H, **f32)
        stat_e = None
        _call("gnm_ln_edge_gate2_fwd", N, E, H, _ptr(t), res_e, _ptr(prm.gamma_e), _ptr(prm.beta_e), lnw, _ptr(P), _ptr(idx["isrc"]),
              _ptr(idx["idst"]), _ptr(idx["in_ptr"]), _ptr(plan["sinfo"]), _ptr(plan["dinfo"]), plan["nodes_per_block"], plan["nfix"],
              _ptr(plan["fix_nodes"]), _ptr(idx["out_ptr"]), _ptr(idx["out_pos"]), _ptr(idx["out_dst"]), _ptr(e_out),
              _ptr(hf), _ptr(inv_f), _ptr(hb), _ptr(inv_b), _ptr(z), _ptr(sc.partials), C.byref(nblk), st)
    elif two_sided:
        hb = torch.empty(N, H, **f32)
        inv_b = torch.empty(N, H, **f32) if save else None
        z = torch.empty(N, H, **f32)
        stat_e = bn_finalize(sc.partials, nblk.value, E, H, prm.gamma_e, prm.beta_e)
        _call("gnm_edge_gate2_fwd", N, E, H, _ptr(t), res_e, _ptr(stat_e), _ptr(P), _ptr(idx["isrc"]), _ptr(idx["idst"]),
              _ptr(idx["in_ptr"]), _ptr(plan["sinfo"]), _ptr(plan["dinfo"]), plan["nodes_per_block"], plan["nfix"],
              _ptr(plan["fix_nodes"]), _ptr(idx["out_ptr"]), _ptr(idx["out_pos"]), _ptr(idx["out_dst"]), _ptr(e_out),
              _ptr(hf), _ptr(inv_f), _ptr(hb), _ptr(inv_b), _ptr(z), _ptr(sc.partials), C.byref(nblk), st)
    elif batch_norm:
        stat_e = bn_finalize(sc.partials, nblk.value, E, H, prm.gamma_e, prm.beta_e)
        _call("gnm_edge_gate_fwd", N, E, H, _ptr(t), res_e, _ptr(stat_e), _ptr(P), _ptr(idx["isrc"]),
              _ptr(idx["in_ptr"]), _ptr(e_out), _ptr(hf), _ptr(inv_f), st)
    else:       # LayerNorm: row statistics inside the kernel, no barrier
        stat_e = None
        _call("gnm_ln_edge_gate_fwd", N, E, H, _ptr(t), res_e, _ptr(prm.gamma_e), _ptr(prm.beta_e), _ptr(P),
              _ptr(idx["isrc"]), _ptr(idx["in_ptr"]), _ptr(e_out), _ptr(hf), _ptr(inv_f), lnw, st)
    # by-source gated mean on the same gate, z, BatchNorm statistics over N (:133-147)
    if not two_sided:
        hb = torch.empty(N, H, **f32)
        inv_b = torch.empty(N, H, **f32)
        z = torch.empty(N, H, **f32)
        _call("gnm_node_agg_src_fwd", N, E, H, _ptr(e_out), _ptr(P), _ptr(idx["out_ptr"]),
              _ptr(idx["out_pos"]), _ptr(idx["out_dst"]), _ptr(hf), _ptr(hb),
              _ptr(inv_b), _ptr(z), _ptr(sc.partials), C.byref(nblk), st)
    h_out = torch.empty(N, H, **f32)
    if batch_norm:
        stat_h = bn_finalize(sc.partials, nblk.value, N, H, prm.gamma_h, prm.beta_h)
        _call("gnm_node_update_fwd", N, H, _ptr(z), _ptr(stat_h), res_h, _ptr(h_out), st)
    else:
        stat_h = None
        _call("gnm_ln_node_update_fwd", N, H, _ptr(z), _ptr(prm.gamma_h), _ptr(prm.beta_h), res_h, _ptr(h_out), lnw, st)
    saved = None
    if save:
        lean = current().ACTIVATIONS == "lean"
        saved = LayerSaved(opts=current(), h_in=h_in, e_in=e_in, P=None if lean else P, t=None if lean else t, stat_e=stat_e, e_out=e_out,
                           hf=hf, inv_f=inv_f, hb=hb, inv_b=inv_b, z=z, stat_h=stat_h, matmul=_lib.get_matmul_mode())
    return h_out, e_out, saved


# A layer wider than the widest kernel instantiation (gated_gcn_full.py:44-50 takes any nn.Linear width): the two dense products
# run at full width on the generic GEMM route, everything between them -- BatchNorm statistics, gate, both aggregations, node
# update, and the duals of all of it -- is separable by columns and runs once per WIDE_CHUNK-column problem on contiguous copies
# of the chunk (strided copies in and out: slow by construction, but a legal width no longer raises).  BatchNorm by default; LayerNorm's
# row statistics span the chunks: _wide_ln_layer_forward below, opt-in (layers.WIDE_LAYERNORM).
WIDE_CHUNK = 256


def _cols(x: torch.Tensor, c0: int, w: int, blocks: int = 1) -> torch.Tensor:
    """Columns c0 .. c0+w of each of the `blocks` equal blocks of x's rows, as a contiguous [rows, blocks*w] tensor."""
    R, Hb = x.shape[0], x.shape[1] // blocks
    return x.view(R, blocks, Hb)[:, :, c0:c0 + w].reshape(R, blocks * w).contiguous()


def _put_cols(dst: torch.Tensor, src: torch.Tensor, c0: int, w: int, blocks: int = 1) -> None:
    R, Hb = dst.shape[0], dst.shape[1] // blocks
    dst.view(R, blocks, Hb)[:, :, c0:c0 + w] = src.view(R, blocks, w)


def _chunk_params(prm: LayerParams, c0: int, w: int) -> LayerParams:
    """The per-channel parameters of one column chunk (the weights are not read behind the dense products)."""
    sl = slice(c0, c0 + w)
    return LayerParams(W5=None, b5=None, W3=None, b3=None, gamma_e=prm.gamma_e[sl], beta_e=prm.beta_e[sl],
                       gamma_h=prm.gamma_h[sl], beta_h=prm.beta_h[sl])


def _wide_ln_enabled(wide_ln: Optional[bool]) -> bool:
    if wide_ln is None:
        from . import layers
        return bool(layers.WIDE_LAYERNORM)
    return bool(wide_ln)


def _wide_layer_forward(idx, N, E, H, prm, h_in, e_in, save, batch_norm, residual, plan, lnw=None, wide_ln=None):
    if not batch_norm and _wide_ln_enabled(wide_ln):
        if H % WIDE_CHUNK:
            raise _lib.GnmError(f"layer_forward: a wide layer runs zero-padded to a multiple of {WIDE_CHUNK} (layers.padded_width), got {H}")
        return _wide_ln_layer_forward(idx, N, E, H, prm, h_in, e_in, save, residual, H if lnw is None else lnw)
    if not batch_norm:
        raise NotImplementedError(f"GatedGCN_1d with LayerNorm at width {H}: the LayerNorm kernels hold a row in one wavefront "
                                  f"(widths up to {WIDE_CHUNK}); BatchNorm layers run at any width")
    if H % WIDE_CHUNK:
        raise _lib.GnmError(f"layer_forward: a wide layer runs zero-padded to a multiple of {WIDE_CHUNK} (layers.padded_width), got {H}")
    dev = h_in.device
    sc = scratch(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    P = torch.empty(N, 5 * H, **f32)
    t = torch.empty(E, H, **f32)
    gemm(NT, h_in, prm.W5, P, bias=prm.b5)                                      # (:107-112)
    gemm(NT, e_in, prm.W3, t, bias=prm.b3)                                      # (:113)
    h_out, e_out = torch.empty(N, H, **f32), torch.empty(E, H, **f32)
    chunks = []
    w = WIDE_CHUNK
    for c0 in range(0, H, w):
        Pc, tc = _cols(P, c0, w, 5), _cols(t, c0, w)
        hc = _cols(h_in, c0, w) if residual else h_in
        ec = _cols(e_in, c0, w) if residual else e_in
        nblk = C.c_int(0)
        _call("gnm_edge_t_stats_fwd", E, w, _ptr(tc), _ptr(Pc), _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(sc.partials), C.byref(nblk),
              _stream())
        ho, eo, sv = _layer_forward_tail(idx, N, E, w, _chunk_params(prm, c0, w), hc, ec, Pc, tc, nblk, save, True, residual, plan, w)
        _put_cols(h_out, ho, c0, w)
        _put_cols(e_out, eo, c0, w)
        if save:
            sv.h_in = sv.e_in = None            # the full-width inputs are kept once, below
            chunks.append(sv)
    saved = LayerSaved(opts=current(), h_in=h_in, e_in=e_in, chunks=chunks, matmul=_lib.get_matmul_mode()) if save else None
    return h_out, e_out, saved


# LayerNorm at a width above 256 (opt-in: layers.WIDE_LAYERNORM).  The same chunking, but a row's statistics span its chunks: the
# forward forms (mean, rstd) of every whole row once (gnm_ln_wide_row_stats over the stack of chunk copies) and hands them to the
# per-chunk gate / node update; the backward sums the two row means of LNbwd chunk by chunk (phase A, ascending chunk order on one
# stream) before any chunk applies them (phase B).  What carries no norm is the BatchNorm path's: gnm_edge_t_stats_fwd (its
# BatchNorm partial sums are ignored), gnm_node_agg_src_fwd, gnm_ln_edge_bwd_src, the GEMM tail.  Separate passes only (no sweep plan).
def _wide_row_stats(stack: torch.Tensor, lnw: int) -> torch.Tensor:
    """(mean, rstd) [R,2] over the lnw live channels of the rows of a [C,R,256] stack of chunk copies."""
    C_, R, w = stack.shape
    stat = torch.empty(R, 2, dtype=torch.float32, device=stack.device)
    _call("gnm_ln_wide_row_stats", R, C_, _ptr(stack), R * w, lnw, _ptr(stat), _stream())
    return stat


def _wide_ln_layer_forward(idx, N, E, H, prm, h_in, e_in, save, residual, lnw):
    dev = h_in.device
    sc = scratch(dev)
    st = _stream()
    f32 = dict(dtype=torch.float32, device=dev)
    w = WIDE_CHUNK
    nc = H // w
    P = torch.empty(N, 5 * H, **f32)
    t = torch.empty(E, H, **f32)
    gemm(NT, h_in, prm.W5, P, bias=prm.b5)                                      # (:107-112)
    gemm(NT, e_in, prm.W3, t, bias=prm.b3)                                      # (:113)
    ts = torch.empty(nc, E, w, **f32)
    Ps = []
    for ci, c0 in enumerate(range(0, H, w)):
        Ps.append(_cols(P, c0, w, 5))
        ts[ci].copy_(t[:, c0:c0 + w])
        _call("gnm_edge_t_stats_fwd", E, w, _ptr(ts[ci]), _ptr(Ps[ci]), _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(sc.partials),
              C.byref(C.c_int(0)), st)                                          # (:120-121)
    del P, t
    stat_e = _wide_row_stats(ts, lnw)
    h_out, e_out = torch.empty(N, H, **f32), torch.empty(E, H, **f32)
    zs = torch.empty(nc, N, w, **f32)
    chunks = []
    for ci, c0 in enumerate(range(0, H, w)):
        cp = _chunk_params(prm, c0, w)
        ec = _cols(e_in, c0, w) if residual else None
        eo, hf, inv_f, hb, inv_b = (torch.empty(E, w, **f32), torch.empty(N, w, **f32), torch.empty(N, w, **f32),
                                    torch.empty(N, w, **f32), torch.empty(N, w, **f32))
        _call("gnm_ln_wide_edge_gate_fwd", N, E, _ptr(ts[ci]), _ptr(ec), _ptr(cp.gamma_e), _ptr(cp.beta_e), _ptr(stat_e), _ptr(Ps[ci]),
              _ptr(idx["isrc"]), _ptr(idx["in_ptr"]), _ptr(eo), _ptr(hf), _ptr(inv_f), c0, lnw, st)        # (:122-130)
        _call("gnm_node_agg_src_fwd", N, E, w, _ptr(eo), _ptr(Ps[ci]), _ptr(idx["out_ptr"]), _ptr(idx["out_pos"]), _ptr(idx["out_dst"]),
              _ptr(hf), _ptr(hb), _ptr(inv_b), _ptr(zs[ci]), _ptr(sc.partials), C.byref(C.c_int(0)), st)   # (:133-147)
        _put_cols(e_out, eo, c0, w)
        if save:
            lean = current().ACTIVATIONS == "lean"
            chunks.append(LayerSaved(P=None if lean else Ps[ci], t=None if lean else ts[ci], e_out=eo, hf=hf, inv_f=inv_f, hb=hb,
                                     inv_b=inv_b, z=zs[ci]))
    stat_h = _wide_row_stats(zs, lnw)
    for ci, c0 in enumerate(range(0, H, w)):
        cp = _chunk_params(prm, c0, w)
        hc = _cols(h_in, c0, w) if residual else None
        ho = torch.empty(N, w, **f32)
        _call("gnm_ln_wide_node_update_fwd", N, _ptr(zs[ci]), _ptr(stat_h), _ptr(cp.gamma_h), _ptr(cp.beta_h), _ptr(hc), _ptr(ho), c0, lnw,
              st)                                                                # (:147-152)
        _put_cols(h_out, ho, c0, w)
    saved = LayerSaved(opts=current(), h_in=h_in, e_in=e_in, chunks=chunks, stat_e=stat_e, stat_h=stat_h,
                       matmul=_lib.get_matmul_mode()) if save else None
    return h_out, e_out, saved


def _wide_ln_layer_backward(idx, N, E, H, prm, s: LayerSaved, gh_out, ge, out, residual, lnw):
    dev = gh_out.device
    sc = scratch(dev)
    st = _stream()
    f32 = dict(dtype=torch.float32, device=dev)
    Hin = s.h_in.shape[1]
    w = WIDE_CHUNK
    new = lambda key, *shape: out[key] if key in out else torch.empty(*shape, **f32)  # noqa: E731
    g: Dict[str, torch.Tensor] = {k: new(k, H) for k in ("gamma_e", "beta_e", "gamma_h", "beta_h")}
    if any(c.P is None or c.t is None for c in s.chunks):      # "lean" activations: the saved stat_e is the forward's
        _wide_rebuild(idx, N, E, H, prm, s)
    nblk = C.c_int(0)
    starts = list(range(0, H, w))
    rs_h = torch.empty(N, 2, **f32)
    rs_e = torch.empty(E, 2, **f32)
    ghc = [_cols(gh_out, c0, w) for c0 in starts]
    # node side, phase A: the row sums of LNbwd_h over all chunks, the column partials of ggamma_h / gbeta_h
    for ci, c0 in enumerate(starts):
        sl, c = slice(c0, c0 + w), s.chunks[ci]
        _call("gnm_ln_wide_node_bwd_sums", N, _ptr(c.z), _ptr(s.stat_h), _ptr(prm.gamma_h[sl]), _ptr(prm.beta_h[sl]), _ptr(ghc[ci]),
              _ptr(rs_h), _ptr(sc.partials), C.byref(nblk), c0, lnw, st)
        bn_bwd_finalize(sc.partials, nblk.value, N, w, dev, g["gamma_h"][sl], g["beta_h"][sl])
    # node side, phase B (gz, Q); edge side, phase A (ge in place, gA3h, the row sums of LNbwd_e, ggamma_e / gbeta_e)
    gPs, Qs, ges = [], [], []
    for ci, c0 in enumerate(starts):
        sl, c = slice(c0, c0 + w), s.chunks[ci]
        gPc, Q, gec = torch.empty(N, 5 * w, **f32), torch.empty(N, 4 * w, **f32), _cols(ge, c0, w)
        _call("gnm_ln_wide_node_bwd_apply", N, _ptr(c.z), _ptr(s.stat_h), _ptr(prm.gamma_h[sl]), _ptr(prm.beta_h[sl]), _ptr(ghc[ci]),
              _ptr(rs_h), _ptr(c.hf), _ptr(c.inv_f), _ptr(c.hb), _ptr(c.inv_b), _ptr(gPc), _ptr(Q), c0, lnw, st)
        _call("gnm_ln_wide_edge_bwd_sums", N, E, _ptr(c.e_out), _ptr(c.t), _ptr(s.stat_e), _ptr(prm.gamma_e[sl]), _ptr(prm.beta_e[sl]),
              _ptr(gec), _ptr(c.P), _ptr(Q), _ptr(idx["isrc"]), _ptr(idx["in_ptr"]), _ptr(gPc), _ptr(rs_e), _ptr(sc.partials),
              C.byref(nblk), c0, lnw, st)
        bn_bwd_finalize(sc.partials, nblk.value, E, w, dev, g["gamma_e"][sl], g["beta_e"][sl])
        gPs.append(gPc), Qs.append(Q), ges.append(gec)
    del ghc
    # edge side, phase B: gt and gB2h with the whole rows' sums, then the by-source pass (gA2h, gB1h)
    gP = torch.empty(N, 5 * H, **f32)
    gt = torch.empty(E, H, **f32)
    ge_tot = ge if residual else None
    for ci, c0 in enumerate(starts):
        sl, c = slice(c0, c0 + w), s.chunks[ci]
        gtc = torch.empty(E, w, **f32)
        _call("gnm_ln_wide_edge_bwd_apply", N, E, _ptr(c.t), _ptr(s.stat_e), _ptr(prm.gamma_e[sl]), _ptr(prm.beta_e[sl]), _ptr(ges[ci]),
              _ptr(rs_e), _ptr(idx["in_ptr"]), _ptr(gtc), _ptr(gPs[ci]), c0, lnw, st)
        _call("gnm_ln_edge_bwd_src", N, E, w, _ptr(c.e_out), _ptr(gtc), _ptr(Qs[ci]), _ptr(idx["out_ptr"]), _ptr(idx["out_pos"]),
              _ptr(idx["out_dst"]), _ptr(gPs[ci]), st)
        _put_cols(gP, gPs[ci], c0, w, 5)
        _put_cols(gt, gtc, c0, w)
        if residual:
            _put_cols(ge_tot, ges[ci], c0, w)
        gPs[ci] = Qs[ci] = ges[ci] = s.chunks[ci] = None
    return _wide_backward_tail(N, E, H, Hin, prm, s, gP, gt, ge_tot, gh_out, g, out, residual)


def _same_matmul_mode(s) -> None:
    """A lean-mode backward rebuilds P and t with the forward's kernels, and the chained / two-sided schedules exist in the split
    modes only: a backward in another matmul mode than its forward would silently mix arithmetic."""
    m = getattr(s, "matmul", None)
    if m is not None and m != _lib.get_matmul_mode():
        raise _lib.GnmError(f"backward in matmul mode {_lib.get_matmul_mode()!r} of a forward that ran in {m!r}: "
                            "gnm_set_matmul_mode is process-wide, change it between steps, not inside one")


def _wide_rebuild(idx, N, E, H, prm, s: LayerSaved) -> None:
    """The lean backward of a wide layer: each chunk's P and t exactly as _wide_layer_forward made them -- both dense products at
    full width, then per chunk the contiguous copy and gnm_edge_t_stats_fwd (its BatchNorm partial sums are not used: the chunk's
    saved stat_e is the forward's).  The full-width P and t are dropped as soon as the chunk copies exist."""
    dev = s.h_in.device
    sc = scratch(dev)
    P = torch.empty(N, 5 * H, dtype=torch.float32, device=dev)
    t = torch.empty(E, H, dtype=torch.float32, device=dev)
    gemm(NT, s.h_in, prm.W5, P, bias=prm.b5)
    gemm(NT, s.e_in, prm.W3, t, bias=prm.b3)
    w = WIDE_CHUNK
    for ci, c0 in enumerate(range(0, H, w)):
        sc_ = s.chunks[ci]
        sc_.P, sc_.t = _cols(P, c0, w, 5), _cols(t, c0, w)
        _call("gnm_edge_t_stats_fwd", E, w, _ptr(sc_.t), _ptr(sc_.P), _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(sc.partials),
              C.byref(C.c_int(0)), _stream())
    del P, t


def _wide_layer_backward(idx, N, E, H, prm, s: LayerSaved, gh_out, ge, out, residual, plan):
    dev = gh_out.device
    f32 = dict(dtype=torch.float32, device=dev)
    Hin = s.h_in.shape[1]
    w = WIDE_CHUNK
    new = lambda key, *shape: out[key] if key in out else torch.empty(*shape, **f32)  # noqa: E731
    g: Dict[str, torch.Tensor] = {k: new(k, H) for k in ("gamma_e", "beta_e", "gamma_h", "beta_h")}
    if any(c.P is None or c.t is None for c in s.chunks):      # "lean" activations: rebuild every chunk's P and t with the
        _wide_rebuild(idx, N, E, H, prm, s)                     # kernels that made them, before the first chunk reads them
    gP = torch.empty(N, 5 * H, **f32)
    gt = torch.empty(E, H, **f32)
    ge_tot = ge if residual else None           # the residual path adds the incoming edge gradient: updated in place, chunk by chunk
    for ci, c0 in enumerate(range(0, H, w)):
        sl = slice(c0, c0 + w)
        sc_ = s.chunks[ci]
        outc = {k: g[k][sl] for k in g}
        gec = _cols(ge, c0, w)
        gPc, gec, bstat_e, _ = _bn_backward_mid(idx, N, E, w, _chunk_params(prm, c0, w), sc_, _cols(gh_out, c0, w), gec, outc, plan)
        gtc = torch.empty(E, w, **f32)
        _call("gnm_edge_bwd_gt", E, w, _ptr(gec), _ptr(sc_.t), _ptr(sc_.stat_e), _ptr(bstat_e), _ptr(prm.gamma_e[sl]), _ptr(gtc), _stream())
        _put_cols(gP, gPc, c0, w, 5)
        _put_cols(gt, gtc, c0, w)
        if residual:
            _put_cols(ge_tot, gec, c0, w)
        s.chunks[ci] = None
    return _wide_backward_tail(N, E, H, Hin, prm, s, gP, gt, ge_tot, gh_out, g, out, residual)


def _wide_backward_tail(N, E, H, Hin, prm, s, gP, gt, ge_tot, gh_out, g, out, residual):
    """The full-width dense products behind the chunks of a wide layer's backward (either norm): B_3 and the five projections."""
    f32 = dict(dtype=torch.float32, device=gh_out.device)
    new = lambda key, *shape: out[key] if key in out else torch.empty(*shape, **f32)  # noqa: E731
    g["W3"] = new("W3", H, Hin)
    g["b3"] = gemm_tn_colsum(gt, s.e_in, g["W3"], out.get("b3"))
    if residual:
        gemm(NN, gt, prm.W3, ge_tot, resid=ge_tot)
        ge_in = ge_tot
    else:
        ge_in = gemm(NN, gt, prm.W3, torch.empty(E, Hin, **f32))
    del gt
    g["W5"] = new("W5", 5 * H, Hin)
    g["b5"] = gemm_tn_colsum(gP, s.h_in, g["W5"], out.get("b5"))
    gh_in = torch.empty(N, Hin, **f32)
    gemm(NN, gP, prm.W5, gh_in, resid=gh_out if residual else None)
    return gh_in, ge_in, g


def _bn_backward_mid(idx, N, E, H, prm, s, gh_out, ge, out, plan):
    """The BatchNorm layer backward between the dense products (column-separable like _layer_forward_tail): BatchNorm_h backward,
    the by-destination and by-source passes.  `ge` ([E,H]) is updated in place to ge_tot = ge + gsigma sigma'.  Returns
    (gP [N,5H], ge, bstat_e, {gamma_h, beta_h, gamma_e, beta_e gradients})."""
    lib = _lib.load()
    dev = gh_out.device
    sc = scratch(dev)
    st = _stream()
    nblk = C.c_int(0)
    f32 = dict(dtype=torch.float32, device=dev)
    g: Dict[str, torch.Tensor] = {}
    gP = torch.empty(N, 5 * H, **f32)
    Q = torch.empty(N, 2 * H, **f32)     # Qf | Qb
    # BatchNorm_h backward statistics, then gz and the per-node gate-gradient factors
    _call("gnm_node_bwd_stats", N, H, _ptr(s.z), _ptr(s.stat_h), _ptr(gh_out), _ptr(sc.partials),
          C.byref(nblk), st)
    bstat_h, g["gamma_h"], g["beta_h"] = bn_bwd_finalize(sc.partials, nblk.value, N, H, dev, out.get("gamma_h"), out.get("beta_h"))
    _call("gnm_node_bwd_apply", N, H, _ptr(s.z), _ptr(s.stat_h), _ptr(bstat_h), _ptr(prm.gamma_h),
          _ptr(gh_out), _ptr(s.inv_f), _ptr(s.inv_b), _ptr(gP), _ptr(Q), st)
    if plan is not None and H in (128, 256) and current().TWO_SIDED:
        # the two-sided sweep of the chained schedule's top layer (H = 256: once per 128-column half, row pitch 256; H = 128:
        # the fp32-MFMA matmul mode, whose edge backward is not chained): by-destination AND by-source sums from one pass over
        # ge, e_out, t; then the unserved sources and the conversion through m1, m2
        UT = torch.empty(N, 2 * H, **f32)
        DT = torch.empty(N, 2 * H, **f32)
        Ud, Td = DT[:, :H], DT[:, H:]
        need_f = lib.gnm_edge_bwd_fused_workspace_bytes()
        ws = sc.ws(need_f)
        _call("gnm_edge_bwd_top", N, E, H, _ptr(ge), _ptr(s.e_out), _ptr(s.t), _ptr(s.stat_e), _ptr(s.P), _ptr(Q), _ptr(s.hf),
              _ptr(s.hb), _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(idx["in_ptr"]), _ptr(gP), _ptr(Ud), _ptr(Td),
              _ptr(sc.partials), _ptr(plan["sinfo"]), plan["nodes_per_block"], _ptr(UT), C.byref(nblk), _ptr(ws), need_f, st)
        _call("gnm_edge_bwd_src_fix", plan["nfix"], _ptr(plan["fix_nodes"]), N, E, H, _ptr(s.e_out), _ptr(s.t),
              _ptr(s.stat_e), _ptr(ge), _ptr(Q), _ptr(idx["out_ptr"]), _ptr(idx["out_pos"]), _ptr(idx["out_dst"]),
              _ptr(gP), _ptr(UT), st)
        bstat_e, g["gamma_e"], g["beta_e"] = bn_bwd_finalize(sc.partials, nblk.value, E, H, dev, out.get("gamma_e"), out.get("beta_e"))
        _call("gnm_node_bgrad", N, H, _ptr(s.stat_e), _ptr(bstat_e), _ptr(prm.gamma_e), _ptr(idx["in_ptr"]),
              _ptr(idx["out_ptr"]), _ptr(UT), _ptr(Ud), _ptr(Td), Ud.stride(0), _ptr(gP), st)
        del UT, DT
    else:
        # by-destination pass: ge <- ge + gsigma*sigma', gA3h, BatchNorm_e backward statistics
        Ud = torch.empty(N, H, **f32)
        Td = torch.empty(N, H, **f32)
        _call("gnm_edge_bwd_dst", N, E, H, _ptr(s.e_out), _ptr(s.t), _ptr(s.stat_e), _ptr(ge), _ptr(s.P),
              _ptr(Q), _ptr(s.hf), _ptr(s.hb), _ptr(idx["isrc"]), _ptr(idx["in_ptr"]), _ptr(gP), _ptr(Ud), _ptr(Td),
              _ptr(sc.partials), C.byref(nblk), st)
        bstat_e, g["gamma_e"], g["beta_e"] = bn_bwd_finalize(sc.partials, nblk.value, E, H, dev, out.get("gamma_e"), out.get("beta_e"))
        # by-source pass: gA2h, gB1h, gB2h
        _call("gnm_edge_bwd_src", N, E, H, _ptr(s.e_out), _ptr(s.t), _ptr(s.stat_e), _ptr(bstat_e),
              _ptr(prm.gamma_e), _ptr(ge), _ptr(Q), _ptr(idx["in_ptr"]), _ptr(idx["out_ptr"]),
              _ptr(idx["out_pos"]), _ptr(idx["out_dst"]), _ptr(Ud), _ptr(Td), _ptr(gP), 0, st)
    del Ud, Td, Q
    return gP, ge, bstat_e, g


@on_device_of(lambda idx, N, E, H, prm, s, gh_out, *a, **k: gh_out)
@_scoped(5)
def layer_backward(idx, N: int, E: int, H: int, prm: LayerParams, s: LayerSaved, gh_out, ge, batch_norm: bool = True,
                   out: Optional[Dict[str, torch.Tensor]] = None, residual: bool = True, plan: Optional[dict] = None,
                   ln_width: Optional[int] = None, lane: Optional[SideLane] = None):
    """Backward of layer_forward.  `ge` ([E,H], internal order) holds d loss / d e_out on entry
    and is OVERWRITTEN with d loss / d e_in (residual layers; without the residual the returned ge is a fresh [E,Hin]
    tensor).  Returns (gh_in, ge, grads dict).  `out` (optional) names the tensors
    the parameter gradients are written INTO (keys W5 b5 W3 b3 gamma_e beta_e gamma_h beta_h; contiguous blocks,
    e.g. views of a flat gradient buffer) instead of fresh allocations.
    lane (H = 128 fused route, H = 256): the weight gradients may run on its side stream; the CALLER then drains it before
    anything reads them (model_backward does, after the last layer).  None: everything on the current stream."""
    out = out or {}
    Hin = s.h_in.shape[1]
    lnw = H if ln_width is None else int(ln_width)
    fused = H == 128 and current().FUSED and residual          # the fused backward kernels have the residual adds built in
    # the two weight-gradient GEMMs of a 256-wide layer on the side stream
    defer_side = lane is not None and H == 256 and batch_norm and _lib.split_mode()
    deferred_first = True
    new = lambda key, *shape: out[key] if key in out else torch.empty(*shape, dtype=torch.float32, device=gh_out.device)  # noqa: E731
    lib = _lib.load()
    dev = gh_out.device
    sc = scratch(dev)
    st = _stream()
    nblk = C.c_int(0)
    f32 = dict(dtype=torch.float32, device=dev)
    g: Dict[str, torch.Tensor] = {}
    _same_matmul_mode(s)
    if s.chunks is not None:
        if not batch_norm:
            return _wide_ln_layer_backward(idx, N, E, H, prm, s, gh_out, ge, out, residual, lnw)
        return _wide_layer_backward(idx, N, E, H, prm, s, gh_out, ge, out, residual, plan)
    if s.P is None or s.t is None:      # "lean" activations: rebuild P and t with the kernels that made them
        s.P, s.t = _proj_and_t(idx, N, E, H, prm, s.h_in, s.e_in, C.c_int(0))
    g["W3"] = new("W3", H, Hin)
    if not batch_norm:
        gP = torch.empty(N, 5 * H, **f32)
        Q = torch.empty(N, 4 * H, **f32)     # LayerNorm mode: Qf | Qb | Rf | Rb
        # ---- LayerNorm mode: no global barriers, gt is produced by the by-destination pass ----
        _call("gnm_ln_node_bwd", N, H, _ptr(s.z), _ptr(prm.gamma_h), _ptr(prm.beta_h), _ptr(gh_out), _ptr(s.hf),
              _ptr(s.inv_f), _ptr(s.hb), _ptr(s.inv_b), _ptr(gP), _ptr(Q), _ptr(sc.partials), C.byref(nblk), lnw, st)
        _, g["gamma_h"], g["beta_h"] = bn_bwd_finalize(sc.partials, nblk.value, N, H, dev, out.get("gamma_h"), out.get("beta_h"))
        gt = torch.empty(E, H, **f32)
        if plan is not None and H == 128 and current().TWO_SIDED and current().LN_SWEEP:
            # round 6: by-destination AND by-source sums from ONE two-sided sweep (the LayerNorm form of the top sweep: gt is complete
            # inside a row, so gB1h / gB2h come out of the sweep directly), then the plan's unserved sources by gathers
            need_f = lib.gnm_edge_bwd_fused_workspace_bytes()
            ws = sc.ws(need_f)
            _call("gnm_ln_edge_bwd_top", N, E, H, _ptr(ge), _ptr(s.e_out), _ptr(s.t), _ptr(prm.gamma_e), _ptr(prm.beta_e), lnw,
                  _ptr(s.P), _ptr(Q), _ptr(s.hf), _ptr(s.hb), _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(idx["in_ptr"]), _ptr(gP), _ptr(gt),
                  _ptr(sc.partials), _ptr(plan["sinfo"]), plan["nodes_per_block"], C.byref(nblk), _ptr(ws), need_f, st)
            _call("gnm_ln_edge_bwd_src_fix", plan["nfix"], _ptr(plan["fix_nodes"]), N, E, H, _ptr(s.e_out), _ptr(gt), _ptr(Q),
                  _ptr(idx["out_ptr"]), _ptr(idx["out_pos"]), _ptr(idx["out_dst"]), _ptr(gP), st)
            _, g["gamma_e"], g["beta_e"] = bn_bwd_finalize(sc.partials, nblk.value, E, H, dev, out.get("gamma_e"), out.get("beta_e"))
        else:
            _call("gnm_ln_edge_bwd_dst", N, E, H, _ptr(s.e_out), _ptr(s.t), _ptr(prm.gamma_e), _ptr(prm.beta_e),
                  _ptr(ge), _ptr(s.P), _ptr(Q), _ptr(idx["isrc"]), _ptr(idx["in_ptr"]), _ptr(gP), _ptr(gt),
                  _ptr(sc.partials), C.byref(nblk), lnw, st)
            _, g["gamma_e"], g["beta_e"] = bn_bwd_finalize(sc.partials, nblk.value, E, H, dev, out.get("gamma_e"), out.get("beta_e"))
            _call("gnm_ln_edge_bwd_src", N, E, H, _ptr(s.e_out), _ptr(gt), _ptr(Q), _ptr(idx["out_ptr"]),
                  _ptr(idx["out_pos"]), _ptr(idx["out_dst"]), _ptr(gP), st)
        del Q
        if fused and Hin == H and _lib.split_mode():
            # round 6: gW3 = gt^T e_in, gb3 = sum gt and ge_in = ge + gt W3 from ONE pass over gt, ge, e_in (the fused edge backward
            # with gt given) instead of gemm_tn_colsum + gemm NN with the residual add
            g["b3"] = new("b3", H)
            need = lib.gnm_edge_bwd_fused_workspace_bytes()
            ws = sc.ws(need)
            _call("gnm_edge_bwd_fused_gt", E, H, _ptr(ge), _ptr(ge), _ptr(gt), _ptr(s.e_in), _ptr(prm.W3), _ptr(g["W3"]), _ptr(g["b3"]),
                  _ptr(sc.partials), _ptr(ws), need, st)
        else:
            g["b3"] = gemm_tn_colsum(gt, s.e_in, g["W3"], out.get("b3"))
            if residual:
                gemm(NN, gt, prm.W3, ge, resid=ge)
            else:
                ge = gemm(NN, gt, prm.W3, torch.empty(E, Hin, **f32))
        del gt
    else:
        gP, ge, bstat_e, gm = _bn_backward_mid(idx, N, E, H, prm, s, gh_out, ge, out, plan)
        g.update(gm)
        # gt, B_3 gradients, ge_in = ge_tot + gt W3
        if fused:
            g["b3"] = new("b3", H)
            need = lib.gnm_edge_bwd_fused_workspace_bytes()
            ws = sc.ws(need)
            _call("gnm_edge_bwd_fused", E, H, _ptr(ge), _ptr(ge), _ptr(s.t), _ptr(s.e_in), _ptr(s.stat_e), _ptr(bstat_e),
                  _ptr(prm.gamma_e), _ptr(prm.W3), _ptr(g["W3"]), _ptr(g["b3"]), _ptr(sc.partials), _ptr(ws), need, st)
        elif H == 256 and current().FUSED and current().WIDE_FUSED and residual and Hin == H and _lib.split_mode():
            # the reference's default width: gt and ge_in = ge_tot + gt W3 from one pass, gt kept for the weight-gradient GEMM
            gt = torch.empty(E, H, **f32)
            ge_in = torch.empty(E, H, **f32)
            need = lib.gnm_rowtile_workspace_bytes(5 * H)
            ws = sc.ws(need)
            _call("gnm_edge_bwd_gt_nn", E, H, _ptr(ge), _ptr(s.t), _ptr(s.stat_e), _ptr(bstat_e), _ptr(prm.gamma_e),
                  _ptr(prm.W3), _ptr(gt), _ptr(ge_in), _ptr(ws), need, st)
            ge = ge_in
            if defer_side:          # round 6: beside the next layer's HBM-bound sweep instead of in front of it
                g["b3"] = new("b3", H)
                lane.begin()
                lane.gemm_tn_colsum(gt, s.e_in, g["W3"], g["b3"])
                deferred_first = False
            else:
                g["b3"] = gemm_tn_colsum(gt, s.e_in, g["W3"], out.get("b3"))
            del gt
        else:
            gt = torch.empty(E, H, **f32)
            _call("gnm_edge_bwd_gt", E, H, _ptr(ge), _ptr(s.t), _ptr(s.stat_e), _ptr(bstat_e),
                  _ptr(prm.gamma_e), _ptr(gt), st)
            g["b3"] = gemm_tn_colsum(gt, s.e_in, g["W3"], out.get("b3"))
            if residual:
                gemm(NN, gt, prm.W3, ge, resid=ge)
            else:
                ge = gemm(NN, gt, prm.W3, torch.empty(E, Hin, **f32))
            del gt
    # node projections backward
    g["W5"] = new("W5", 5 * H, Hin)
    gh_in = torch.empty(N, Hin, **f32)
    if fused:
        g["b5"] = new("b5", 5 * H)
        need = lib.gnm_node_proj_bwd_workspace_bytes(5 * H)
        ws = sc.ws(need)
        _call("gnm_node_proj_bwd_nn", N, H, 5 * H, _ptr(gP), _ptr(prm.W5), _ptr(gh_out), _ptr(gh_in), _ptr(ws), need, st)
        if lane is not None:
            # the weight gradient has no consumer before the optimizer step: on the side stream, beside the next layer's HBM-bound
            # node / by-destination passes (what the chained schedule does with its deferred kernel)
            lane.begin()
            lane.node_proj_bwd_tn(N, H, gP, s.h_in, g["W5"], g["b5"])
        else:
            _call("gnm_node_proj_bwd_tn", N, H, 5 * H, _ptr(gP), _ptr(s.h_in), _ptr(g["W5"]), _ptr(g["b5"]),
                  _ptr(sc.partials), _ptr(ws), need, 0, st)
    else:
        gemm(NN, gP, prm.W5, gh_in, resid=gh_out if residual else None)
        if defer_side:
            g["b5"] = new("b5", 5 * H)
            lane.begin() if deferred_first else lane.wait_for_main()
            lane.gemm_tn_colsum(gP, s.h_in, g["W5"], g["b5"])
        else:
            g["b5"] = gemm_tn_colsum(gP, s.h_in, g["W5"], out.get("b5"))
    return gh_in, ge, g


# The chained backward schedule (H = 128, BatchNorm, the split matmul modes): the fused edge backward of layer i runs in
# ONE kernel with the by-destination pass of layer i-1 (gnm_edge_bwd_chain: 5 [E,H] streams instead of 4 + 4, the
# matrix-core work under the gather arithmetic).  GNM_CHAIN=0 / engine.options(CHAIN=False) goes back to layer_backward.
_D_CHAIN = os.environ.get("GNM_CHAIN", "1") != "0"
# Inside the chained schedule: layer i's node-projection weight gradient (gW5 = gP^T h_in, matrix-core bound, no consumer
# before the optimizer step) is launched on a side stream BESIDE layer i-1's by-source pass (HBM bound), which is capped
# at four workgroups per CU (4 x 80 registers per SIMD lane) so that the weight-gradient workgroups (168 registers) find
# room on every CU.  Measured on one box: 187.9 -> 183.8 ms/step; with five by-source workgroups the two kernels no
# longer co-reside and nothing is gained.  The caps travel as ARGUMENTS of the two launches (max_blocks_per_cu; 0 = none):
# no process-wide state is touched (round 2 flipped gnm_set_occupancy_cap between the launches, and the weight-gradient
# kernel never honoured it: TN_SIDE_CAP = 0 is what was measured).  GNM_TN_SIDE=0 keeps everything on one stream (the
# per-op timing mode always does).
_D_TN_SIDE = os.environ.get("GNM_TN_SIDE", "1") != "0"
_D_TN_SIDE_CAP = int(os.environ.get("GNM_TN_CAP", "0"))
# when the deferred weight-gradient kernel of layer i is launched: "next" = at the head of layer i-1's iteration (beside its
# by-source pass / conversion), "now" = right after layer i's own by-source pass or conversion (beside nn(i), node(i-1))
# "auto" (default): by graph size -- "now" from TN_AT_NOW_NODES nodes on, "next" below.  At the metric's graph (N = 1.5 M) "now" wins
# (161.4 vs 163.2 ms/step bf16x3, 153.6-154.2 vs 154.8-155.4 f16x2: profiles/r05_ab_tn_at.txt, r05_ab_schedule_f16x2.txt); on small graphs the
# HBM-bound window beside nn(i) / node(i-1) is too short for the weight-gradient kernel and "next" wins: N = 750 k 76.8-77.7 vs 77.4-79.0 ms,
# N = 220 k (the true chr19 size) 24.6-24.7 vs 24.8-24.9, the mini-batch epoch (sub-graphs of N = 150 k) 41.5-42.1 vs 40.5-41.3 M edges/s
# (profiles/r05_ab_tn_at_sizes.txt)
_D_TN_AT = os.environ.get("GNM_TN_AT", "auto")
TN_AT_NOW_NODES = int(os.environ.get("GNM_TN_AT_NOW_NODES", "1100000"))


def tn_at(N: int) -> str:
    """The TN_AT switch of the current options resolved for a graph of N nodes ("auto": by size, see TN_AT_NOW_NODES)."""
    v = current().TN_AT
    return ("now" if N >= TN_AT_NOW_NODES else "next") if v == "auto" else v
# "next" only: the deferred kernel in TWO launches sized to the two HBM-bound windows of an iteration -- the gB1h | gB2h column groups
# beside this layer's conversion (node_bgrad), the gA1h | gA2h | gA3h groups AFTER this layer's nn (both matrix bound: side by side
# they only take turns) beside the next layer's BatchNorm_h backward.  GNM_TN_SPLIT=0: one launch at the head of the iteration.
_D_TN_SPLIT = os.environ.get("GNM_TN_SPLIT", "1") != "0"
_D_SRC_SIDE_CAP = int(os.environ.get("GNM_SRC_CAP", "4"))


# The chained kernel as a TWO-SIDED sweep (gnm_edge_bwd_chain_src): layer i-1's by-source sums (gA2h, Us, Ts) come out of the
# same pass through the graph's sweep plan (graph.sweep_plan), the separate by-source pass -- three [E,H] streams re-read per
# layer -- shrinks to a gather over the few per cent of the nodes the plan does not serve plus an [N,H]-sized conversion
# once the BatchNorm-backward means are known.  GNM_TWO_SIDED=0 / engine.options(TWO_SIDED=False) keeps the separate pass.
_D_TWO_SIDED = os.environ.get("GNM_TWO_SIDED", "1") != "0"
# the forward twin (gnm_edge_gate2_fwd): gate + by-destination AND by-source aggregation in one sweep; GNM_TWO_SIDED_FWD=0
# keeps edge_gate_fwd + node_agg_src_fwd
_D_TWO_SIDED_FWD = os.environ.get("GNM_TWO_SIDED_FWD", "1") != "0"
# H = 256 (the reference's default width): the fused forward kernel for t (gnm_edge_t_fused_fwd at H = 256);
# GNM_WIDE_FUSED=0 keeps gemm NT + edge_t_stats_fwd
_D_WIDE_FUSED = os.environ.get("GNM_WIDE_FUSED", "1") != "0"


# Round 5, the node side.  (A pre-split image of h -- the kernel that produces h also writes its three bf16 terms, the projections
# and their weight gradient copy them instead of splitting the rows in every workgroup class -- was built, measured at +1.4 ms per
# step, profiles/r05_ab_node_side.txt, and removed again when the f16x2 mode made its bf16x3 layout the wrong one: DESIGN.md 3g.)
# NODE_FUSED (chained schedule with a sweep plan): no gnm_node_bgrad / gnm_node_bwd_stats launches -- the conversion of the raw
# by-source / by-destination sums runs in the operand load of the weight-gradient kernel of those two column groups
# (gnm_tn128_bgrad, which also writes them for the projection backward behind it), the BatchNorm_h backward sums of the layer
# below in the epilogue of the projection backward (gnm_node_proj_bwd_nn_stats).  GNM_NODE_FUSED=0: the round-4 schedule.
_D_NODE_FUSED = os.environ.get("GNM_NODE_FUSED", "1") != "0"
# Round 6, LayerNorm models at H = 128 with a sweep plan: the backward's by-destination and by-source passes as ONE two-sided sweep
# (gnm_ln_edge_bwd_top + gnm_ln_edge_bwd_src_fix).  GNM_LN_SWEEP=0: gnm_ln_edge_bwd_dst + gnm_ln_edge_bwd_src.
_D_LN_SWEEP = os.environ.get("GNM_LN_SWEEP", "1") != "0"


def tn128(N: int, A: torch.Tensor, lda: int, ncg: int, h: torch.Tensor, W, b, partials, ws, need, tag: str = None):
    """gW[cg] = A[:, cg]^T h, gb[cg] = sum A[:, cg] (gnm_tn128) on the current stream (SideLane.tn128: on the side stream)."""
    _call("gnm_tn128", N, _ptr(A), lda, ncg, _ptr(h), _ptr(W), _ptr(b), _ptr(partials), _ptr(ws), need, _stream(), tag=tag)


# workgroups per CU of the two-sided forward sweep (the partition its plan is built for); 1 only together with
# GNM_VARIANTS=gate2_wg=1: the occupancy experiment of profiles/r06_ab_gate2_occupancy.txt
GATE2_WG = int(os.environ.get("GNM_GATE2_WG", "2"))


def sweep_width(H: int, batch_norm: bool = True) -> bool:
    """Does a layer of (kernel) width H run the two-sided sweeps?  128; with BatchNorm also 256 (one sweep per 128-column half) and
    the wide layers (256-column chunks)."""
    return H == 128 or (batch_norm and (H == 256 or (H > WIDE_CHUNK and H % WIDE_CHUNK == 0)))


def chain_eligible(H: int, batch_norm: bool) -> bool:
    return current().CHAIN and current().FUSED and H == 128 and batch_norm and _lib.split_mode()


def layers_backward_chained(idx, N: int, E: int, H: int, P: Dict[str, torch.Tensor], L: int, saved: List[LayerSaved],
                            gh, ge, outs: List[Optional[Dict[str, torch.Tensor]]], plan: Optional[dict] = None,
                            lane: Optional[SideLane] = None, first: int = 0, mask=None):
    """Backward of the L-layer stack (layers L-1 .. 0), same arithmetic as L x layer_backward, other schedule:
        node(L-1), dst(L-1);   then for i = L-1 .. 0:   finalize_e(i), src(i), proj(i),
                                                         i > 0:  node(i-1), CHAIN[fused(i) + dst(i-1)]
                                                         i = 0:  fused(0)
    `ge` is updated in place through all layers.  Returns (gh_in of layer 0, ge_in of layer 0, [grads dict per layer]);
    saved[i] is released as soon as layer i is done.  outs[i]: write-into targets as in layer_backward (or None).
    With `plan` (graph.sweep_plan) the chained kernel is the two-sided sweep: src(i) for i < L-1 becomes
    fix(i) [right after CHAIN(i+1, i)] + bgrad(i) [after finalize_e(i)].  With `lane` the node-projection weight gradients run on
    its side stream (TN_AT, TN_SPLIT say when); the caller drains it.
    first: the stack is the model's layers first .. first+L-1 (a checkpoint segment: `saved` and `outs` hold those L layers, the
    parameters are read at the offset); its top layer is treated like a model's top layer, its bottom layer like layer 0.
    mask (node-output dropout, p > 0): mask(layer, gh) applies that model layer's dropout mask to the gradient of its output IN
    PLACE; every layer's node backward is preceded by it.  Not with NODE_FUSED, which forms the BatchNorm_h backward sums of the
    unmasked gradient inside the projection backward (model_forward pins it off: _dropout_opts)."""
    lib = _lib.load()
    dev = gh.device
    sc, sc2 = scratch(dev), scratch(dev, "chain")     # sc2: the chained kernel's second partials buffer
    st = _stream()
    f32 = dict(dtype=torch.float32, device=dev)
    grads: List[Dict[str, torch.Tensor]] = [dict() for _ in range(L)]
    prms = [None] * L

    def tgt(i, key, *shape):
        o = outs[i] or {}
        return o[key] if key in o else torch.empty(*shape, **f32)

    def ensure(i):
        if prms[i] is None:
            prms[i] = layer_params(P, first + i)
        s = saved[i]
        if s.P is None or s.t is None:      # "lean" activations
            s.P, s.t = _proj_and_t(idx, N, E, H, prms[i], s.h_in, s.e_in, C.c_int(0))
        return prms[i], s

    def node(i, gh_out, nblk_h=None):
        """BatchNorm_h backward of layer i -> gP[:, 0:H] = gz, Q = Qf | Qb.  nblk_h: the (sum gw, sum gw zhat) partials are in
        the scratch buffer already (the projection backward of the layer above took them in its epilogue: NODE_FUSED)."""
        prm, s = ensure(i)
        o = outs[i] or {}
        gP = torch.empty(N, 5 * H, **f32)
        Q = torch.empty(N, 2 * H, **f32)
        if mask is not None:
            mask(first + i, gh_out)
        if nblk_h is None:
            nblk_h = C.c_int(0)
            _call("gnm_node_bwd_stats", N, H, _ptr(s.z), _ptr(s.stat_h), _ptr(gh_out), _ptr(sc.partials), C.byref(nblk_h), st)
        bstat_h, grads[i]["gamma_h"], grads[i]["beta_h"] = bn_bwd_finalize(sc.partials, nblk_h.value, N, H, dev,
                                                                          o.get("gamma_h"), o.get("beta_h"))
        _call("gnm_node_bwd_apply", N, H, _ptr(s.z), _ptr(s.stat_h), _ptr(bstat_h), _ptr(prm.gamma_h),
              _ptr(gh_out), _ptr(s.inv_f), _ptr(s.inv_b), _ptr(gP), _ptr(Q), st)
        return gP, Q

    need_f = lib.gnm_edge_bwd_fused_workspace_bytes()
    need_p = lib.gnm_node_proj_bwd_workspace_bytes(5 * H)
    need_t = lib.gnm_tn128_workspace_bytes()
    i = L - 1
    prm, s = ensure(i)
    gP, Q = node(i, gh)
    nblk = C.c_int(0)
    UT = None                   # two-sided sweep: the raw by-source sums [Us | Ts] of the current layer (None: src(i) forms them)
    if plan is None:
        Ud, Td = torch.empty(N, H, **f32), torch.empty(N, H, **f32)
        _call("gnm_edge_bwd_dst", N, E, H, _ptr(s.e_out), _ptr(s.t), _ptr(s.stat_e), _ptr(ge), _ptr(s.P),
              _ptr(Q), _ptr(s.hf), _ptr(s.hb), _ptr(idx["isrc"]), _ptr(idx["in_ptr"]), _ptr(gP), _ptr(Ud), _ptr(Td),
              _ptr(sc.partials), C.byref(nblk), st)
    else:                       # the top layer on the same two-sided sweep as the chained kernel (no layer above)
        UT = torch.empty(N, 2 * H, **f32)
        DT = torch.empty(N, 2 * H, **f32)
        Ud, Td = DT[:, :H], DT[:, H:]
        ws = sc.ws(max(need_p, need_f, need_t))
        _call("gnm_edge_bwd_top", N, E, H, _ptr(ge), _ptr(s.e_out), _ptr(s.t), _ptr(s.stat_e), _ptr(s.P), _ptr(Q), _ptr(s.hf),
              _ptr(s.hb), _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(idx["in_ptr"]), _ptr(gP), _ptr(Ud), _ptr(Td),
              _ptr(sc.partials), _ptr(plan["sinfo"]), plan["nodes_per_block"], _ptr(UT), C.byref(nblk), _ptr(ws), need_f, st)
        _call("gnm_edge_bwd_src_fix", plan["nfix"], _ptr(plan["fix_nodes"]), N, E, H, _ptr(s.e_out), _ptr(s.t),
              _ptr(s.stat_e), _ptr(ge), _ptr(Q), _ptr(idx["out_ptr"]), _ptr(idx["out_pos"]), _ptr(idx["out_dst"]),
              _ptr(gP), _ptr(UT), st)
    if current().ACTIVATIONS == "lean":
        s.P = None              # as below: only the by-destination pass reads the rebuilt P
    # not in the lean mode: the deferred kernel keeps its gP (one [E,H]-sized tensor) alive one layer longer
    fusedn = current().NODE_FUSED and plan is not None      # the node side without node_bgrad / node_bwd_stats launches (see NODE_FUSED)
    if fusedn and mask is not None:
        raise _lib.GnmError("node-output dropout cannot run under NODE_FUSED (the projection backward would take the BatchNorm_h "
                            "backward sums of the unmasked gradient): run the backward under the options its forward saved")
    at_now = tn_at(N) == "now"          # when the deferred weight-gradient kernel is launched (TN_AT; "auto": by graph size)
    pending = None              # (gP, h_in, gW5, gb5) of the layer above: its weight-gradient kernel, not yet launched
    pending2 = None             # the same, when only its first launch (TN_SPLIT) has been issued
    while True:
        prm, s = prms[i], saved[i]
        o = outs[i] or {}
        g = grads[i]
        bstat_e, g["gamma_e"], g["beta_e"] = bn_bwd_finalize(sc.partials, nblk.value, E, H, dev, o.get("gamma_e"), o.get("beta_e"))
        g["W5"], g["b5"] = tgt(i, "W5", 5 * H, H), tgt(i, "b5", 5 * H)
        gh_in = torch.empty(N, H, **f32)
        ws = sc.ws(max(need_p, need_f, need_t))
        nblk_h = None
        if fusedn:
            # ---- round 5: tn34(i) [forms gB1h | gB2h from the raw sums, writes them to gP, their weight gradient] ->
            #      nn(i) [+ the BatchNorm_h backward sums of layer i-1 in its epilogue];  the weight gradient of the other three
            #      column groups on the side stream beside the HBM-bound BatchNorm_h backward of layer i-1
            if pending is not None:         # tn012 of the layer above, deferred (TN_AT = "next")
                lane.begin()
                lane.tn128(N, pending[0], 5 * H, 3, *pending[1:])
                pending = None
            _call("gnm_tn128_bgrad", N, H, _ptr(UT), _ptr(Ud), _ptr(Td), Ud.stride(0), _ptr(s.stat_e), _ptr(bstat_e),
                  _ptr(prm.gamma_e), _ptr(idx["in_ptr"]), _ptr(idx["out_ptr"]), _ptr(gP),
                  _ptr(s.h_in), _ptr(g["W5"][3 * H:]), _ptr(g["b5"][3 * H:]),
                  _ptr(sc.partials), _ptr(ws), need_t, st)
            del Ud, Td, Q
            UT = None
            if i > 0:
                s_j = ensure(i - 1)[1]
                nblk_h = C.c_int(0)
                _call("gnm_node_proj_bwd_nn_stats", N, H, 5 * H, _ptr(gP), _ptr(prm.W5), _ptr(gh), _ptr(gh_in), _ptr(s_j.z),
                      _ptr(s_j.stat_h), _ptr(sc.partials), C.byref(nblk_h), _ptr(ws), need_p, st)
            else:
                _call("gnm_node_proj_bwd_nn", N, H, 5 * H, _ptr(gP), _ptr(prm.W5), _ptr(gh), _ptr(gh_in), _ptr(ws), need_p, st)
            if lane is not None and at_now:             # tn012(i) right away, beside node(i-1)'s [N,H] passes
                lane.begin()
                lane.tn128(N, gP, 5 * H, 3, s.h_in, g["W5"], g["b5"])
            elif lane is not None and i > 0:
                pending = (gP, s.h_in, g["W5"], g["b5"])
            else:       # no side stream (lean activations, per-op timing) or the last iteration: the same launch on this stream
                sw = sc if nblk_h is None else scratch(dev, "wgrad")    # (sc.partials holds layer i-1's BatchNorm_h sums)
                tn128(N, gP, 5 * H, 3, s.h_in, g["W5"], g["b5"], sw.partials, sw.ws(need_t), need_t, tag="gnm_tn128[3]")
        else:
            src_cap = 0
            if pending is not None:
                # the matrix-bound weight gradient of the layer above on the side stream, beside this layer's HBM-bound
                # by-source pass (see TN_SIDE)
                pgP, ph, pW, pb = pending
                lane.begin()
                if current().TN_SPLIT and UT is not None:
                    lane.tn128(N, pgP[:, 3 * H:], 5 * H, 2, ph, pW[3 * H:], pb[3 * H:])
                    pending2 = pending
                else:
                    lane.node_proj_bwd_tn(N, H, *pending)
                pending = None
                src_cap = current().SRC_SIDE_CAP
            if UT is None:
                _call("gnm_edge_bwd_src", N, E, H, _ptr(s.e_out), _ptr(s.t), _ptr(s.stat_e), _ptr(bstat_e),
                      _ptr(prm.gamma_e), _ptr(ge), _ptr(Q), _ptr(idx["in_ptr"]), _ptr(idx["out_ptr"]),
                      _ptr(idx["out_pos"]), _ptr(idx["out_dst"]), _ptr(Ud), _ptr(Td), _ptr(gP), src_cap, st)
            else:       # the sums are there (chain_src + fix): only the conversion through m1, m2 is left
                _call("gnm_node_bgrad", N, H, _ptr(s.stat_e), _ptr(bstat_e), _ptr(prm.gamma_e), _ptr(idx["in_ptr"]),
                      _ptr(idx["out_ptr"]), _ptr(UT), _ptr(Ud), _ptr(Td), Ud.stride(0), _ptr(gP), st)
            split2 = UT is not None
            del Ud, Td, Q
            UT = None
            if not (lane is not None and at_now):
                _call("gnm_node_proj_bwd_nn", N, H, 5 * H, _ptr(gP), _ptr(prm.W5), _ptr(gh), _ptr(gh_in), _ptr(ws), need_p, st)
            if pending2 is not None:        # the other three column groups of the layer above, behind this layer's nn
                lane.wait_for_main()
                lane.tn128(N, pending2[0], 5 * H, 3, *pending2[1:])
                pending2 = None
            if lane is not None and at_now:
                lane.begin()
                lane.node_proj_bwd_tn(N, H, gP, s.h_in, g["W5"], g["b5"])
                _call("gnm_node_proj_bwd_nn", N, H, 5 * H, _ptr(gP), _ptr(prm.W5), _ptr(gh), _ptr(gh_in), _ptr(ws), need_p, st)
            elif lane is not None and i > 0:
                pending = (gP, s.h_in, g["W5"], g["b5"])
            elif lane is None and i > 0 and current().TN_SPLIT and split2:
                # no side stream (lean activations, per-op timing): the same two launches the deferred path issues, back to back --
                # the row partition of a launch depends on its column-group count, and the two modes must stay bit-identical
                ws_t = sc.ws(max(need_p, need_f, need_t))
                tn128(N, gP[:, 3 * H:], 5 * H, 2, s.h_in, g["W5"][3 * H:], g["b5"][3 * H:], sc.partials, ws_t, need_t,
                      tag="gnm_node_proj_bwd_tn")
                tn128(N, gP, 5 * H, 3, s.h_in, g["W5"], g["b5"], sc.partials, ws_t, need_t, tag="gnm_node_proj_bwd_tn")
            else:
                _call("gnm_node_proj_bwd_tn", N, H, 5 * H, _ptr(gP), _ptr(s.h_in), _ptr(g["W5"]), _ptr(g["b5"]),
                      _ptr(sc.partials), _ptr(ws), need_p, 0, st)
        del gP
        gh = gh_in
        g["W3"], g["b3"] = tgt(i, "W3", H, H), tgt(i, "b3", H)
        if i == 0:
            _call("gnm_edge_bwd_fused", E, H, _ptr(ge), _ptr(ge), _ptr(s.t), _ptr(s.e_in), _ptr(s.stat_e), _ptr(bstat_e),
                  _ptr(prm.gamma_e), _ptr(prm.W3), _ptr(g["W3"]), _ptr(g["b3"]), _ptr(sc.partials), _ptr(ws), need_f, st)
            saved[0] = None
            break
        j = i - 1
        prm_j, s_j = ensure(j)
        gP, Q = node(j, gh, nblk_h)
        if plan is None:
            Ud, Td = torch.empty(N, H, **f32), torch.empty(N, H, **f32)
            _call("gnm_edge_bwd_chain", N, E, H, _ptr(ge), _ptr(ge), _ptr(s.t), _ptr(s.e_in), _ptr(s.stat_e), _ptr(bstat_e),
                  _ptr(prm.gamma_e), _ptr(prm.W3), _ptr(g["W3"]), _ptr(g["b3"]), _ptr(sc2.partials),
                  _ptr(s_j.t), _ptr(s_j.stat_e), _ptr(s_j.P), _ptr(Q), _ptr(s_j.hf), _ptr(s_j.hb),
                  _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(idx["in_ptr"]), _ptr(gP), _ptr(Ud), _ptr(Td), _ptr(sc.partials),
                  C.byref(nblk), _ptr(ws), need_f, st)
        else:
            UT = torch.empty(N, 2 * H, **f32)
            DT = torch.empty(N, 2 * H, **f32)       # [Ud | Td] in one array (the run-sum variant stores both through one buffer)
            Ud, Td = DT[:, :H], DT[:, H:]
            _call("gnm_edge_bwd_chain_src", N, E, H, _ptr(ge), _ptr(ge), _ptr(s.t), _ptr(s.e_in), _ptr(s.stat_e), _ptr(bstat_e),
                  _ptr(prm.gamma_e), _ptr(prm.W3), _ptr(g["W3"]), _ptr(g["b3"]), _ptr(sc2.partials),
                  _ptr(s_j.t), _ptr(s_j.stat_e), _ptr(s_j.P), _ptr(Q), _ptr(s_j.hf), _ptr(s_j.hb),
                  _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(idx["in_ptr"]), _ptr(gP), _ptr(Ud), _ptr(Td), _ptr(sc.partials),
                  _ptr(plan["sinfo"]), plan["nodes_per_block"], _ptr(UT), C.byref(nblk), _ptr(ws), need_f, st)
            # the sources the plan does not serve (chunk boundaries, repeat edges, no out-edges): ge holds ge_tot(j) now
            _call("gnm_edge_bwd_src_fix", plan["nfix"], _ptr(plan["fix_nodes"]), N, E, H, _ptr(s_j.e_out), _ptr(s_j.t),
                  _ptr(s_j.stat_e), _ptr(ge), _ptr(Q), _ptr(idx["out_ptr"]), _ptr(idx["out_pos"]), _ptr(idx["out_dst"]),
                  _ptr(gP), _ptr(UT), st)
        saved[i] = None         # release layer i's activations
        if current().ACTIVATIONS == "lean":
            s_j.P = None        # rebuilt for the by-destination pass only; nothing after it reads P
        i = j
    return gh, ge, grads


def ln_chain_eligible(H: int, batch_norm: bool) -> bool:
    """The chained LayerNorm backward (round 6): H = 128, split matmul modes, the two-sided LayerNorm sweep switched on."""
    o = current()
    return (not batch_norm) and o.CHAIN and o.FUSED and o.TWO_SIDED and o.LN_SWEEP and H == 128 and _lib.split_mode()


def layers_backward_chained_ln(idx, N: int, E: int, H: int, P: Dict[str, torch.Tensor], L: int, saved: List[LayerSaved], gh, ge,
                               outs: List[Optional[Dict[str, torch.Tensor]]], plan: dict, lnw: int, lane: Optional[SideLane] = None,
                               first: int = 0, mask=None):
    """Backward of an L-layer LayerNorm stack (batch_norm=False), chained like layers_backward_chained.  LayerNorm has no global
    statistics, so the schedule is shorter than BatchNorm's -- no finalisation between a layer's passes, no conversion of raw sums:
        node(L-1), sweep(L-1) [+ fix];   then for i = L-1 .. 0:   nn(i), tn(i) [side stream],
                                              i > 0:  node(i-1), CHAIN[fused(i) with gt(i) given + sweep(i-1)] [+ fix(i-1)]
                                              i = 0:  fused(0) with gt(0) given
    The sweep of layer i writes gt(i) once; the chained kernel of the next iteration reads it back as layer i's given gt (6 [E,H]
    streams per layer where the layer-by-layer schedule moves 9).  Returns (gh_in of layer 0, ge_in of layer 0, [grads dict per layer]).
    With `lane` tn(i) runs on its side stream; the caller drains it.  first, mask: as in layers_backward_chained."""
    lib = _lib.load()
    dev = gh.device
    sc, sc2 = scratch(dev), scratch(dev, "chain")
    st = _stream()
    f32 = dict(dtype=torch.float32, device=dev)
    grads: List[Dict[str, torch.Tensor]] = [dict() for _ in range(L)]
    prms = [None] * L
    need_f = lib.gnm_edge_bwd_fused_workspace_bytes()
    need_p = lib.gnm_node_proj_bwd_workspace_bytes(5 * H)

    def tgt(i, key, *shape):
        o = outs[i] or {}
        return o[key] if key in o else torch.empty(*shape, **f32)

    def ensure(i):
        if prms[i] is None:
            prms[i] = layer_params(P, first + i)
        s = saved[i]
        _same_matmul_mode(s)
        if s.P is None or s.t is None:      # "lean" activations
            s.P, s.t = _proj_and_t(idx, N, E, H, prms[i], s.h_in, s.e_in, C.c_int(0))
        return prms[i], s

    def node(i, gh_out):
        prm, s = ensure(i)
        o = outs[i] or {}
        gP = torch.empty(N, 5 * H, **f32)
        Q = torch.empty(N, 4 * H, **f32)
        nb = C.c_int(0)
        if mask is not None:
            mask(first + i, gh_out)
        _call("gnm_ln_node_bwd", N, H, _ptr(s.z), _ptr(prm.gamma_h), _ptr(prm.beta_h), _ptr(gh_out), _ptr(s.hf),
              _ptr(s.inv_f), _ptr(s.hb), _ptr(s.inv_b), _ptr(gP), _ptr(Q), _ptr(sc.partials), C.byref(nb), lnw, st)
        _, grads[i]["gamma_h"], grads[i]["beta_h"] = bn_bwd_finalize(sc.partials, nb.value, N, H, dev, o.get("gamma_h"), o.get("beta_h"))
        return gP, Q

    def fix_and_finalize(j, s_j, gt_j, Q_j, gP_j, nblk):
        o = outs[j] or {}
        _call("gnm_ln_edge_bwd_src_fix", plan["nfix"], _ptr(plan["fix_nodes"]), N, E, H, _ptr(s_j.e_out), _ptr(gt_j), _ptr(Q_j),
              _ptr(idx["out_ptr"]), _ptr(idx["out_pos"]), _ptr(idx["out_dst"]), _ptr(gP_j), st)
        _, grads[j]["gamma_e"], grads[j]["beta_e"] = bn_bwd_finalize(sc.partials, nblk.value, E, H, dev, o.get("gamma_e"), o.get("beta_e"))

    i = L - 1
    prm, s = ensure(i)
    gP, Q = node(i, gh)
    gt = torch.empty(E, H, **f32)
    nblk = C.c_int(0)
    ws = sc.ws(max(need_f, need_p))
    _call("gnm_ln_edge_bwd_top", N, E, H, _ptr(ge), _ptr(s.e_out), _ptr(s.t), _ptr(prm.gamma_e), _ptr(prm.beta_e), lnw,
          _ptr(s.P), _ptr(Q), _ptr(s.hf), _ptr(s.hb), _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(idx["in_ptr"]), _ptr(gP), _ptr(gt),
          _ptr(sc.partials), _ptr(plan["sinfo"]), plan["nodes_per_block"], C.byref(nblk), _ptr(ws), need_f, st)
    fix_and_finalize(i, s, gt, Q, gP, nblk)
    del Q
    while True:
        prm, s = prms[i], saved[i]
        g = grads[i]
        g["W5"], g["b5"] = tgt(i, "W5", 5 * H, H), tgt(i, "b5", 5 * H)
        gh_in = torch.empty(N, H, **f32)
        ws = sc.ws(max(need_f, need_p))
        _call("gnm_node_proj_bwd_nn", N, H, 5 * H, _ptr(gP), _ptr(prm.W5), _ptr(gh), _ptr(gh_in), _ptr(ws), need_p, st)
        if lane is not None:
            lane.begin()
            lane.node_proj_bwd_tn(N, H, gP, s.h_in, g["W5"], g["b5"])
        else:
            _call("gnm_node_proj_bwd_tn", N, H, 5 * H, _ptr(gP), _ptr(s.h_in), _ptr(g["W5"]), _ptr(g["b5"]), _ptr(sc.partials), _ptr(ws),
                  need_p, 0, st)
        del gP
        gh = gh_in
        g["W3"], g["b3"] = tgt(i, "W3", H, H), tgt(i, "b3", H)
        if i == 0:
            _call("gnm_edge_bwd_fused_gt", E, H, _ptr(ge), _ptr(ge), _ptr(gt), _ptr(s.e_in), _ptr(prm.W3), _ptr(g["W3"]), _ptr(g["b3"]),
                  _ptr(sc.partials), _ptr(ws), need_f, st)
            saved[0] = None
            break
        j = i - 1
        prm_j, s_j = ensure(j)
        gP, Q = node(j, gh)
        gt_j = torch.empty(E, H, **f32)
        ws = sc.ws(max(need_f, need_p))
        _call("gnm_ln_edge_bwd_chain", N, E, H, _ptr(ge), _ptr(gt), _ptr(s.e_in), _ptr(prm.W3), _ptr(g["W3"]), _ptr(g["b3"]),
              _ptr(sc2.partials), _ptr(s_j.t), _ptr(prm_j.gamma_e), _ptr(prm_j.beta_e), lnw, _ptr(s_j.P), _ptr(Q), _ptr(s_j.hf),
              _ptr(s_j.hb), _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(idx["in_ptr"]), _ptr(gP), _ptr(gt_j), _ptr(sc.partials),
              _ptr(plan["sinfo"]), plan["nodes_per_block"], C.byref(nblk), _ptr(ws), need_f, st)
        fix_and_finalize(j, s_j, gt_j, Q, gP, nblk)
        del Q
        saved[i] = None         # release layer i's activations
        if current().ACTIVATIONS == "lean":
            s_j.P = None
        gt = gt_j
        i = j
    return gh, ge, grads


# ---------------------------------------------------------------------------------------
# predictor (score_predictor.py:12-25), split-W1 form
# ---------------------------------------------------------------------------------------

@dataclass
class PredSaved:
    x: torch.Tensor = None
    e: torch.Tensor = None
    hid: torch.Tensor = None     # pre-activation [E,HS]; overwritten by its gradient in backward
    W1sd: torch.Tensor = None
    opts: "Options" = None
    pieces: list = None          # hidden_edge_scores run as padded pieces: [((c0, w, wp), PredSaved of the piece)] (pred_pieces)


PRED_WIDTHS = (32, 64, 128, 256)      # the hidden_edge_scores the predictor's row kernels are built for (GNM_DISPATCH_W)


def pred_pieces(HS: int):
    """[(c0, w, wp)]: the column pieces predictor_forward runs hidden_edge_scores = HS as.  A built width runs as itself; any
    other HS as pieces of at most 256 columns, each zero-padded to the next built width (zero rows of W1 and b1, zero columns
    of W2: relu(0) * 0 adds nothing to the score, and the padded rows' gradients are dropped).  nn.Linear takes any size
    (score_predictor.py:8-9), and so does this."""
    if HS in PRED_WIDTHS:
        return [(0, HS, HS)]
    out = []
    for c0 in range(0, HS, PRED_WIDTHS[-1]):
        w = min(PRED_WIDTHS[-1], HS - c0)
        out.append((c0, w, next(k for k in PRED_WIDTHS if k >= w)))
    return out


def _pred_piece(t, c0, w, wp, cols: bool = False):
    """Rows c0 .. c0+w of W1 [HS,3H] / b1 [HS], or (cols) columns of W2 [1,HS], zero-padded to wp."""
    if cols:
        return torch.nn.functional.pad(t[:, c0:c0 + w], (0, wp - w))
    return torch.nn.functional.pad(t[c0:c0 + w], (0, 0, 0, wp - w) if t.dim() == 2 else (0, wp - w))


@on_device_of(lambda idx, N, E, H, W1, b1, W2, b2, x, *a, **k: x)
@_scoped()
def predictor_forward(idx, N, E, H, W1, b1, W2, b2, x, e, save: bool):
    """scores (caller edge-id order, [E,1]) from internal-order x [N,H], e [E,H].  Any hidden_edge_scores: see pred_pieces."""
    pieces = pred_pieces(W1.shape[0])
    if len(pieces) == 1 and pieces[0][1] == pieces[0][2]:
        return _predictor_forward(idx, N, E, H, W1, b1, W2, b2, x, e, save)
    scores, saved = None, []
    for j, (c0, w, wp) in enumerate(pieces):
        s_j, ps = _predictor_forward(idx, N, E, H, _pred_piece(W1, c0, w, wp), _pred_piece(b1, c0, w, wp),
                                     _pred_piece(W2, c0, w, wp, cols=True), b2 if j == 0 else torch.zeros_like(b2), x, e, save)
        scores = s_j if scores is None else scores.add_(s_j)
        saved.append(ps)
    return scores, (PredSaved(x=x, e=e, opts=current(), pieces=list(zip(pieces, saved))) if save else None)


def _predictor_forward(idx, N, E, H, W1, b1, W2, b2, x, e, save: bool):
    lib = _lib.load()
    dev = x.device
    HS = W1.shape[0]
    f32 = dict(dtype=torch.float32, device=dev)
    W1sd = torch.cat((W1[:, :H], W1[:, H:2 * H]), 0).contiguous()     # [2HS, H]
    Pn = torch.empty(N, 2 * HS, **f32)
    gemm(NT, x, W1sd, Pn)
    scores = torch.empty(E, 1, **f32)
    if (H == 128 or (H == 256 and current().WIDE_FUSED)) and HS == 64 and current().FUSED:
        # one pass over e: hid GEMM + gathers + relu + W2 dot; hid is only written when backward needs it
        hid = torch.empty(E, HS, **f32) if save else None
        need = lib.gnm_predictor_fused_workspace_bytes()
        ws = scratch(dev).ws(need)
        W1e = W1[:, 2 * H:]
        _call("gnm_predictor_fused_fwd", E, H, HS, _ptr(e), _ptr(W1e), W1.stride(0), _ptr(b1), _ptr(Pn),
              _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(idx["perm"]), _ptr(W2), _ptr(b2), _ptr(hid), _ptr(scores),
              _ptr(ws), need, _stream())
    else:
        hid = torch.empty(E, HS, **f32)
        gemm(NT, e, W1[:, 2 * H:], hid, bias=b1)
        _call("gnm_predictor_score_fwd", E, HS, _ptr(hid), _ptr(Pn), _ptr(idx["isrc"]), _ptr(idx["idst"]),
                                               _ptr(W2), _ptr(b2), _ptr(idx["perm"]), _ptr(scores), _stream())
    saved = PredSaved(x=x, e=e, hid=hid, W1sd=W1sd, opts=current()) if save else None
    return scores, saved


@on_device_of(lambda idx, N, E, H, W1, W2, s, gscores, *a, **k: gscores)
@_scoped(6)
def predictor_backward(idx, N, E, H, W1, W2, s: PredSaved, gscores, out: Optional[Dict[str, torch.Tensor]] = None):
    """Returns (gx [N,H], ge [E,H] fresh buffer, grads dict W1,b1,W2,b2); `out` as in layer_backward."""
    if s.pieces is None:
        return _predictor_backward(idx, N, E, H, W1, W2, s, gscores, out)
    # the pieces of predictor_forward: each backward needs only gscores; the padded rows' gradients are dropped
    out = out or {}
    HS = W1.shape[0]
    f32 = dict(dtype=torch.float32, device=gscores.device)
    g = {"W1": out["W1"] if "W1" in out else torch.empty(HS, 3 * H, **f32),
         "b1": out["b1"] if "b1" in out else torch.empty(HS, **f32),
         "W2": out["W2"] if "W2" in out else torch.empty(1, HS, **f32)}
    gx = ge = None
    for (c0, w, wp), ps in s.pieces:
        gx_j, ge_j, g_j = _predictor_backward(idx, N, E, H, _pred_piece(W1, c0, w, wp), _pred_piece(W2, c0, w, wp, cols=True), ps,
                                              gscores)
        g["W1"][c0:c0 + w] = g_j["W1"][:w]
        g["b1"][c0:c0 + w] = g_j["b1"][:w]
        g["W2"][:, c0:c0 + w] = g_j["W2"][:, :w]
        if gx is None:
            gx, ge = gx_j, ge_j
            g["b2"] = out["b2"].copy_(g_j["b2"]) if "b2" in out else g_j["b2"]
        else:
            gx.add_(gx_j)
            ge.add_(ge_j)
    return gx, ge, g


def _predictor_backward(idx, N, E, H, W1, W2, s: PredSaved, gscores, out: Optional[Dict[str, torch.Tensor]] = None):
    out = out or {}
    lib = _lib.load()
    dev = s.x.device
    sc = scratch(dev)
    HS = W1.shape[0]
    st = _stream()
    nblk = C.c_int(0)
    f32 = dict(dtype=torch.float32, device=dev)
    g = {}
    gscores = _f32c(gscores.reshape(-1))
    ghid = s.hid   # in place
    fused = (H == 128 or (H == 256 and current().WIDE_FUSED)) and HS == 64 and current().FUSED
    gW1 = out["W1"] if "W1" in out else torch.empty(HS, 3 * H, **f32)
    if fused:
        # one pass: ghid (in place), ge = ghid W1e, gW1e, and the gW2 / gb1 / gb2 column sums
        ge = torch.empty(E, H, **f32)
        gW1e = torch.empty(HS, H, **f32)
        gsums = torch.empty(3 * HS, **f32)
        need = lib.gnm_predictor_fused_workspace_bytes()
        ws = sc.ws(need)
        _call("gnm_predictor_fused_bwd", E, H, HS, _ptr(ghid), _ptr(gscores), _ptr(idx["perm"]), _ptr(W2), _ptr(s.e),
              _ptr(W1[:, 2 * H:]), W1.stride(0), _ptr(ge), _ptr(gW1e), _ptr(gsums), _ptr(sc.partials), _ptr(ws), need, st)
        def keep(key, src):
            if key in out:
                out[key].copy_(src.reshape(out[key].shape))
                return out[key]
            return src.clone()
        g["W2"] = keep("W2", gsums[0:HS].reshape(1, HS))
        g["b1"] = keep("b1", gsums[HS:2 * HS])
        g["b2"] = keep("b2", gsums[2 * HS:2 * HS + 1])
        gW1[:, 2 * H:] = gW1e
    else:
        _call("gnm_predictor_score_bwd", E, HS, _ptr(ghid), _ptr(gscores), _ptr(W2), _ptr(idx["perm"]),
                                               _ptr(sc.partials), C.byref(nblk), st)
        red = torch.empty(2, HS, **f32)
        _call("gnm_reduce_partials", _ptr(sc.partials), nblk.value, 2, HS, _ptr(red), st)
        g["W2"] = out["W2"].copy_(red[0:1]) if "W2" in out else red[0:1].clone()
        g["b2"] = out["b2"].copy_(red[1, 0:1]) if "b2" in out else red[1, 0:1].clone()
        g["b1"] = colsum(ghid, out.get("b1"))
    gPn = torch.empty(N, 2 * HS, **f32)
    _call("gnm_seg_sum_rows", N, HS, _ptr(ghid), _ptr(idx["out_ptr"]), _ptr(idx["out_pos"]),
                                    _ptr(gPn), 2 * HS, st)
    _call("gnm_seg_sum_rows", N, HS, _ptr(ghid), _ptr(idx["in_ptr"]), C.c_void_p(0),
                                    _ptr(gPn[:, HS:]), 2 * HS, st)
    if fused:
        # [x^T gPs | x^T gPd] in one W-free TN pass (x's 128-column groups against the 128-wide gPn), then transpose the H x 128 result
        xt = torch.empty(H, 2 * HS, **f32)
        junk = torch.empty(H, **f32)
        need = lib.gnm_tn128_workspace_bytes()
        ws = sc.ws(need)
        _call("gnm_tn128", N, _ptr(s.x), H, H // 128, _ptr(gPn), _ptr(xt), _ptr(junk), _ptr(sc.partials), _ptr(ws), need, st)
        gW1[:, :H] = xt[:, :HS].t()
        gW1[:, H:2 * H] = xt[:, HS:].t()
    else:
        gemm(TN, gPn[:, :HS], s.x, gW1[:, :H])
        gemm(TN, gPn[:, HS:], s.x, gW1[:, H:2 * H])
        gemm(TN, ghid, s.e, gW1[:, 2 * H:])
    g["W1"] = gW1
    gx = torch.empty(N, H, **f32)
    gemm(NN, gPn, s.W1sd, gx)
    if not fused:
        ge = torch.empty(E, H, **f32)
        gemm(NN, ghid, W1[:, 2 * H:], ge)
    return gx, ge, g


# ---------------------------------------------------------------------------------------
# whole model (full_graph.py:22-29)
# ---------------------------------------------------------------------------------------

@dataclass
class ModelSaved:
    pe: torch.Tensor = None
    e_int: torch.Tensor = None
    a1: torch.Tensor = None
    e_raw: torch.Tensor = None
    layers: List[LayerSaved] = field(default_factory=list)
    pred: PredSaved = None
    opts: "Options" = None
    matmul: str = None
    checkpoint: int = 0          # k > 0: `layers` stays empty, the backward recomputes the stack in segments of k layers ...
    boundaries: list = field(default_factory=list)      # ... from the (h_in, e_in) of every segment's first layer, kept here
    wide_ln: Optional[bool] = None      # model_forward's wide_ln (LayerNorm above 256 channels): the recomputation runs under the same
    dropout: Optional[tuple] = None     # (p, key, step) of the forward's node-output dropout (p > 0), or None: the backward's masks


def _checkpoint_arg(k) -> int:
    """model_forward's `checkpoint` argument as an int >= 0, or GnmError."""
    try:
        k = operator.index(k)       # int, numpy integer, ...; not 1.5, not "4"
    except TypeError:
        k = -1
    if k < 0:
        raise _lib.GnmError("checkpoint: expected an integer >= 0 (0: keep every layer's activations; k: keep the inputs of "
                            "every k-th layer and recompute the rest in the backward)")
    return k


def checkpoint_segments(num_layers: int, k) -> List[tuple]:
    """The layer segments [(first, last_exclusive), ...] of activation checkpointing with segments of k layers: the last one may
    be shorter, k >= num_layers is one segment, k = 0 (no checkpointing) is no segment."""
    k = _checkpoint_arg(k)
    return [(a, min(a + k, num_layers)) for a in range(0, num_layers, k)] if k else []


def stacked(ts):
    """cat(ts, 0) -- as a VIEW when the tensors already sit back to back in one storage (parameters and gradients
    flattened by models.flatten_parameters / dp.FlatGradients), which saves the copy kernel per layer and pass."""
    t0 = ts[0]
    adjacent = all(t.is_contiguous() and t.dtype == t0.dtype and t.shape[1:] == t0.shape[1:] for t in ts) and all(
        a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
        and a.data_ptr() + a.numel() * a.element_size() == b.data_ptr() for a, b in zip(ts[:-1], ts[1:]))
    if not adjacent:
        return torch.cat(ts, 0)
    rows = sum(t.shape[0] for t in ts)
    size = (rows,) + tuple(t0.shape[1:])
    stride = t0.stride()
    return torch.as_strided(t0, size, stride)


def layer_params(P: Dict[str, torch.Tensor], i: int) -> LayerParams:
    p = f"gnn.convs.{i}."
    return LayerParams(
        W5=stacked([P[p + k + ".weight"] for k in LIN5]),
        b5=stacked([P[p + k + ".bias"] for k in LIN5]),
        W3=P[p + "B_3.weight"], b3=P[p + "B_3.bias"],
        gamma_e=P[p + "bn_e.weight"], beta_e=P[p + "bn_e.bias"],
        gamma_h=P[p + "bn_h.weight"], beta_h=P[p + "bn_h.bias"])


@on_device_of(lambda graph, e_raw, pe, *a, **k: pe)
@_scoped()
def model_forward(graph, e_raw, pe, P: Dict[str, torch.Tensor], num_layers: int, save: bool, batch_norm: bool = True,
                  ln_width: Optional[int] = None, checkpoint: int = 0, wide_ln: Optional[bool] = None, dropout=None):
    """GraphGatedGCNModel.forward.  e_raw [E,edge_features] in edge-id order, pe [N,nb_pos_enc+2].
    Returns (scores [E,1] in edge-id order, ModelSaved or None).  ln_width, wide_ln: see layer_forward.
    checkpoint = k > 0 (with save): layer-segment activation checkpointing -- of the layer stack only the (h_in, e_in) entering
    every k-th layer is kept; model_backward re-runs one segment's forward (same kernels, same inputs: the same bits) right
    before that segment's backward.  The scores are those of checkpoint = 0; without `save` it has no effect.
    dropout = (p, key, step) with p > 0: every layer's node output (the last layer's included) is dropped IN PLACE right behind
    the layer (gated_gcn_full.py:154) with the mask of (key, step, layer, caller's node id, channel) -- no backward kernel reads
    the undropped rows -- and the saved state carries the triple for the backward and the recomputation.  None / p = 0: no launch."""
    checkpoint = _checkpoint_arg(checkpoint)
    drop = _dropout_arg(dropout)
    if drop is not None and _dropout_opts(current()) is not current():
        # p > 0: the whole pass -- what it saves per layer included -- under the pinned switches (see _dropout_opts)
        with use(_dropout_opts(current())):
            return model_forward(graph, e_raw, pe, P, num_layers, save, batch_norm, ln_width=ln_width, checkpoint=checkpoint,
                                 wide_ln=wide_ln, dropout=drop)
    lib = _lib.load()
    dev = pe.device
    _chk_dev(e_raw, pe)
    idx = graph.index(dev)
    N, E = graph.num_nodes(), graph.num_edges()
    H = P["linear_pe.weight"].shape[0]
    f32 = dict(dtype=torch.float32, device=dev)
    pe = node_rows_in(idx, _f32c(pe))         # caller's node numbering -> internal (graph.py "Node numbering")
    e_raw = _f32c(e_raw)
    # encoders                                                            (full_graph.py:23-26)
    h = torch.empty(N, H, **f32)
    gemm(NT, pe, P["linear_pe.weight"], h, bias=P["linear_pe.bias"])
    Fe, Q = e_raw.shape[1], P["linear1_edge.weight"].shape[0]
    fused_enc = current().FUSED and (H == 128 or (H == 256 and current().WIDE_FUSED)) and Fe == 2 and Q == 16
    e = torch.empty(E, H, **f32)
    e_int = a1 = None
    if fused_enc:
        _call("gnm_edge_encoder_fwd", E, H, Fe, Q, _ptr(e_raw), _ptr(idx["perm"]), _ptr(P["linear1_edge.weight"]),
              _ptr(P["linear1_edge.bias"]), _ptr(P["linear2_edge.weight"]), _ptr(P["linear2_edge.bias"]),
              _ptr(e), _stream())
    else:
        e_int = torch.empty(E, Fe, **f32)
        _call("gnm_gather_rows_f32", E, Fe, _ptr(e_raw), _ptr(idx["perm"]), _ptr(e_int), _stream())
        a1 = torch.empty(E, Q, **f32)
        gemm(NT, e_int, P["linear1_edge.weight"], a1, bias=P["linear1_edge.bias"], relu=True)
        gemm(NT, a1, P["linear2_edge.weight"], e, bias=P["linear2_edge.bias"])
    ms = ModelSaved(pe=pe, e_int=e_int, a1=a1, e_raw=e_raw, opts=current(), matmul=_lib.get_matmul_mode()) if save else None
    if save:
        ms.wide_ln = wide_ln        # a checkpointed backward recomputes its layers under the same decision
    if save and drop is not None:
        ms.dropout = drop           # the backward's and the recomputation's masks
    real_w = H if ln_width is None else int(ln_width)               # the mask function's H: the model's real width
    plan2 = graph.sweep_plan(dev, GATE2_WG) if (current().TWO_SIDED_FWD and sweep_width(H, batch_norm) and hasattr(graph, "sweep_plan")) else None
    if save and checkpoint:
        ms.checkpoint = checkpoint
        firsts = {a for a, _ in checkpoint_segments(num_layers, checkpoint)}
        for i in range(num_layers):
            if i in firsts:
                ms.boundaries.append((h, e))
            h, e, _ = layer_forward(idx, N, E, H, layer_params(P, i), h, e, False, batch_norm, plan=plan2, ln_width=ln_width,
                                    wide_ln=wide_ln)
            if drop is not None:
                node_dropout(h, drop, i, real_w, idx.get("nperm"))
    else:
        for i in range(num_layers):
            h, e, ls = layer_forward(idx, N, E, H, layer_params(P, i), h, e, save, batch_norm, plan=plan2, ln_width=ln_width,
                                     wide_ln=wide_ln)
            if drop is not None:
                node_dropout(h, drop, i, real_w, idx.get("nperm"))
            if save:
                ms.layers.append(ls)
    scores, ps = predictor_forward(idx, N, E, H, P["predictor.W1.weight"], P["predictor.W1.bias"],
                                   P["predictor.W2.weight"], P["predictor.W2.bias"], h, e, save)
    if save:
        ms.pred = ps
    return scores, ms


def grad_targets(out: Dict[str, torch.Tensor], i: int) -> Optional[Dict[str, torch.Tensor]]:
    """The write-into map of layer_backward for layer i from per-parameter gradient tensors, if the five stacked
    weights / biases are back to back (they are in dp.FlatGradients over a flattened model); else None."""
    p = f"gnn.convs.{i}."
    w = [out[p + k + ".weight"] for k in LIN5]
    b = [out[p + k + ".bias"] for k in LIN5]
    W5, b5 = stacked(w), stacked(b)
    if W5.data_ptr() != w[0].data_ptr() or b5.data_ptr() != b[0].data_ptr():
        return None
    return {"W5": W5, "b5": b5, "W3": out[p + "B_3.weight"], "b3": out[p + "B_3.bias"],
            "gamma_e": out[p + "bn_e.weight"], "beta_e": out[p + "bn_e.bias"],
            "gamma_h": out[p + "bn_h.weight"], "beta_h": out[p + "bn_h.bias"]}


@on_device_of(lambda graph, P, num_layers, ms, gscores, *a, **k: gscores)
@_scoped(3)
def model_backward(graph, P: Dict[str, torch.Tensor], num_layers: int, ms: ModelSaved, gscores, batch_norm: bool = True,
                   out: Optional[Dict[str, torch.Tensor]] = None, ln_width: Optional[int] = None, inputs: bool = False):
    """Gradients of every parameter (keys = state_dict keys) from d loss / d scores.  With `out` (state_dict key ->
    contiguous tensor of the parameter's shape, e.g. the .grad views of dp.FlatGradients) the kernels write the
    gradients straight into those tensors and the same tensors are returned.  inputs=True: returns (G, g_e_raw, g_pe)
    instead, the gradients of model_forward's inputs -- e_raw [E,edge_features] in the caller's edge-id order, pe
    [N,nb_pos_enc+2] in the caller's node numbering (the encoders' input gradients; inputs=False launches exactly what
    it launched before the option existed).  A checkpointed forward (ms.checkpoint = k > 0): per segment of k layers, from the top, the
    segment's forward again from its kept boundary, then its backward (ms.checkpoint = 0 launches exactly what it launched before).
    One backward at a time per device: the main stream's scratch (`scratch`) is
    shared, so concurrent backward passes on one device are not supported."""
    dev = ms.pe.device
    _same_matmul_mode(ms)
    idx = graph.index(dev)
    N, E = graph.num_nodes(), graph.num_edges()
    H = P["linear_pe.weight"].shape[0]
    f32 = dict(dtype=torch.float32, device=dev)
    G: Dict[str, torch.Tensor] = {}
    tgt = (lambda k, like: out[k]) if out else (lambda k, like: torch.empty_like(like))    # noqa: E731
    pout = {"W1": out["predictor.W1.weight"], "b1": out["predictor.W1.bias"], "W2": out["predictor.W2.weight"],
            "b2": out["predictor.W2.bias"]} if out else None
    gh, ge, gp = predictor_backward(idx, N, E, H, P["predictor.W1.weight"], P["predictor.W2.weight"],
                                    ms.pred, gscores, pout)
    G["predictor.W1.weight"], G["predictor.W1.bias"] = gp["W1"], gp["b1"]
    G["predictor.W2.weight"], G["predictor.W2.bias"] = gp["W2"], gp["b2"]
    ms.pred = None
    louts = [grad_targets(out, i) if out else None for i in range(num_layers)]
    # node-output dropout: the gradient of layer i's output passes through layer i's mask, in place, before its node backward
    mask = None
    if ms.dropout is not None:
        if current().NODE_FUSED:        # an explicit opts= that undoes the forward's pin: see _dropout_opts
            raise _lib.GnmError("model_backward: a forward with node-output dropout cannot be followed by a backward under "
                                "NODE_FUSED; run it under the options the forward saved (ms.opts)")
        real_w, nperm = (H if ln_width is None else int(ln_width)), idx.get("nperm")
        mask = lambda layer, g: node_dropout(g, ms.dropout, layer, real_w, nperm)       # noqa: E731
    # layer-by-layer backward on the two-sided sweep (the chained schedule's top-layer kernel for every layer): H = 256, and H = 128
    # where the chained schedule does not apply (fp32-MFMA matmul mode, GNM_CHAIN=0)
    plan_w = graph.sweep_plan(dev) if (sweep_width(H, batch_norm) and current().TWO_SIDED and not chain_eligible(H, batch_norm)
                                       and hasattr(graph, "sweep_plan")) else None
    # the side stream for the weight gradients (TN_SIDE; not under per-op timing, not with lean activations)
    lane = SideLane(dev) if (current().TN_SIDE and _prof is None and current().ACTIVATIONS != "lean") else None
    # checkpointed forward: one segment at a time from the top -- its forward again from the kept boundary (under the forward's
    # options and matmul mode, which this pass runs in), then its backward on the schedule a whole model of that shape would get
    segs = checkpoint_segments(num_layers, ms.checkpoint) if ms.checkpoint else [(0, num_layers)]
    plan2 = (graph.sweep_plan(dev, GATE2_WG) if (ms.checkpoint and current().TWO_SIDED_FWD and sweep_width(H, batch_norm)
                                                 and hasattr(graph, "sweep_plan")) else None)
    grads = [None] * num_layers
    try:
        for si in reversed(range(len(segs))):
            a, b = segs[si]
            if ms.checkpoint:
                h, e = ms.boundaries[si]
                ms.boundaries[si] = None        # the recomputed first layer keeps them until its own backward is done
                layers = []
                for i in range(a, b):
                    h, e, ls = layer_forward(idx, N, E, H, layer_params(P, i), h, e, True, batch_norm, plan=plan2, ln_width=ln_width,
                                             wide_ln=ms.wide_ln)
                    layers.append(ls)
                    if mask is not None and i < b - 1:      # what the next layer of the segment reads (and keeps as its h_in)
                        mask(i, h)
                del h, e, ls
            else:
                layers = ms.layers
            if chain_eligible(H, batch_norm):
                plan = graph.sweep_plan(dev) if current().TWO_SIDED and hasattr(graph, "sweep_plan") else None
                gh, ge, grads[a:b] = layers_backward_chained(idx, N, E, H, P, b - a, layers, gh, ge, louts[a:b], plan, lane, first=a, mask=mask)
            elif ln_chain_eligible(H, batch_norm) and plan_w is not None:
                gh, ge, grads[a:b] = layers_backward_chained_ln(idx, N, E, H, P, b - a, layers, gh, ge, louts[a:b], plan_w,
                                                                H if ln_width is None else int(ln_width), lane, first=a, mask=mask)
            else:
                for i in reversed(range(a, b)):
                    if mask is not None:
                        mask(i, gh)
                    gh, ge, grads[i] = layer_backward(idx, N, E, H, layer_params(P, i), layers[i - a], gh, ge, batch_norm, louts[i],
                                                      plan=plan_w, ln_width=ln_width, lane=lane)
                    layers[i - a] = None    # release this layer's activations
            del layers
            if lane is not None and si > 0:
                # a deferred weight-gradient kernel of the segment's bottom layer still reads its activations: the lane holds them
                # until the main stream has waited for it -- here, so that they are gone before the next segment is recomputed
                lane.drain()
    finally:
        if lane is not None:
            lane.drain()        # before anything reads a weight gradient, and on the way out of an error
    for i in reversed(range(num_layers)):
        p = f"gnn.convs.{i}."
        gl = grads[i]
        for j, k in enumerate(LIN5):
            G[p + k + ".weight"] = gl["W5"][j * H:(j + 1) * H]
            G[p + k + ".bias"] = gl["b5"][j * H:(j + 1) * H]
        if out and louts[i] is None:      # the caller's targets are not stacked: copy the two stacked results over
            for j, k in enumerate(LIN5):
                G[p + k + ".weight"] = out[p + k + ".weight"].copy_(G[p + k + ".weight"])
                G[p + k + ".bias"] = out[p + k + ".bias"].copy_(G[p + k + ".bias"])
            for key, name in (("W3", "B_3.weight"), ("b3", "B_3.bias"), ("gamma_e", "bn_e.weight"), ("beta_e", "bn_e.bias"),
                              ("gamma_h", "bn_h.weight"), ("beta_h", "bn_h.bias")):
                gl[key] = out[p + name].copy_(gl[key])
        G[p + "B_3.weight"], G[p + "B_3.bias"] = gl["W3"], gl["b3"]
        G[p + "bn_e.weight"], G[p + "bn_e.bias"] = gl["gamma_e"], gl["beta_e"]
        G[p + "bn_h.weight"], G[p + "bn_h.bias"] = gl["gamma_h"], gl["beta_h"]
    # encoders backward
    lib = _lib.load()
    G["linear_pe.weight"] = tgt("linear_pe.weight", P["linear_pe.weight"])
    G["linear_pe.bias"] = gemm_tn_colsum(gh, ms.pe, G["linear_pe.weight"], out["linear_pe.bias"] if out else None)
    g_e_raw = g_pe = None
    if inputs:          # d pe = gh W_pe (full_graph.py:23), internal node numbering -> the caller's
        g_pe = node_rows_out(idx, gemm(NN, gh, P["linear_pe.weight"], torch.empty(N, ms.pe.shape[1], **f32)))
    G["linear2_edge.weight"] = tgt("linear2_edge.weight", P["linear2_edge.weight"])
    G["linear1_edge.weight"] = tgt("linear1_edge.weight", P["linear1_edge.weight"])
    if ms.a1 is None:      # fused encoder: every encoder gradient from one pass over ge
        G["linear2_edge.bias"] = tgt("linear2_edge.bias", P["linear2_edge.bias"])
        G["linear1_edge.bias"] = tgt("linear1_edge.bias", P["linear1_edge.bias"])
        need = lib.gnm_edge_encoder_bwd_workspace_bytes()
        ws = scratch(dev).ws(need)
        if inputs:      # the same pass also writes d e_raw, straight into the caller's edge-id order
            g_e_raw = torch.empty_like(ms.e_raw)
            _call("gnm_edge_encoder_bwd_dx", E, H, ms.e_raw.shape[1], P["linear1_edge.weight"].shape[0], _ptr(ge),
                  _ptr(ms.e_raw), _ptr(idx["perm"]), _ptr(P["linear1_edge.weight"]), _ptr(P["linear1_edge.bias"]),
                  _ptr(P["linear2_edge.weight"]), _ptr(G["linear1_edge.weight"]), _ptr(G["linear1_edge.bias"]),
                  _ptr(G["linear2_edge.weight"]), _ptr(G["linear2_edge.bias"]), _ptr(g_e_raw), _ptr(ws), need, _stream())
        else:
            _call("gnm_edge_encoder_bwd", E, H, ms.e_raw.shape[1], P["linear1_edge.weight"].shape[0], _ptr(ge),
                  _ptr(ms.e_raw), _ptr(idx["perm"]), _ptr(P["linear1_edge.weight"]), _ptr(P["linear1_edge.bias"]),
                  _ptr(P["linear2_edge.weight"]), _ptr(G["linear1_edge.weight"]), _ptr(G["linear1_edge.bias"]),
                  _ptr(G["linear2_edge.weight"]), _ptr(G["linear2_edge.bias"]), _ptr(ws), need, _stream())
    else:
        gemm(TN, ge, ms.a1, G["linear2_edge.weight"])
        G["linear2_edge.bias"] = colsum(ge, out["linear2_edge.bias"] if out else None)
        ga1 = torch.empty_like(ms.a1)
        gemm(NN, ge, P["linear2_edge.weight"], ga1)
        _call("gnm_relu_mask_f32", ga1.numel(), _ptr(ga1), _ptr(ms.a1), _stream())
        gemm(TN, ga1, ms.e_int, G["linear1_edge.weight"])
        G["linear1_edge.bias"] = colsum(ga1, out["linear1_edge.bias"] if out else None)
        if inputs:      # d e_raw = ga1 W1e in internal order, then gathered back to edge-id order
            g_int = gemm(NN, ga1, P["linear1_edge.weight"], torch.empty_like(ms.e_int))
            g_e_raw = torch.empty_like(g_int)
            _call("gnm_gather_rows_f32", E, g_int.shape[1], _ptr(g_int), _ptr(edge_rank(idx)), _ptr(g_e_raw), _stream())
    return (G, g_e_raw, g_pe) if inputs else G


# ---------------------------------------------------------------------------------------
# the layer stack alone (processor.py:15-20): what layers.GraphGatedGCN runs when its node-output dropout is on
# ---------------------------------------------------------------------------------------

@dataclass
class StackSaved:
    layers: List[LayerSaved] = field(default_factory=list)
    dropout: Optional[tuple] = None
    opts: "Options" = None


@on_device_of(lambda idx, N, E, H, P, num_layers, h, *a, **k: h)
@_scoped()
def stack_forward(idx, N: int, E: int, H: int, P: Dict[str, torch.Tensor], num_layers: int, h, e, save: bool, batch_norm: bool = True,
                  ln_width: Optional[int] = None, wide_ln: Optional[bool] = None, dropout=None):
    """GraphGatedGCN.forward on internal-order tensors h [N,H], e [E,H] (P: 'gnn.convs.<i>.' keys as in model_forward): layer
    after layer, each node output through node_dropout (dropout = (p, key, step), as in model_forward).  Returns (h, e, StackSaved
    or None)."""
    drop = _dropout_arg(dropout)
    real_w = H if ln_width is None else int(ln_width)
    ss = StackSaved(dropout=drop, opts=current()) if save else None
    for i in range(num_layers):
        h, e, ls = layer_forward(idx, N, E, H, layer_params(P, i), h, e, save, batch_norm, ln_width=ln_width, wide_ln=wide_ln)
        if drop is not None:
            node_dropout(h, drop, i, real_w, idx.get("nperm"))
        if save:
            ss.layers.append(ls)
    return h, e, ss


@on_device_of(lambda idx, N, E, H, P, num_layers, ss, gh, *a, **k: gh)
@_scoped(6)
def stack_backward(idx, N: int, E: int, H: int, P: Dict[str, torch.Tensor], num_layers: int, ss: StackSaved, gh, ge,
                   batch_norm: bool = True, ln_width: Optional[int] = None):
    """Backward of stack_forward, layer by layer.  gh [N,H] is read (never written), ge [E,H] is OVERWRITTEN as in layer_backward.
    Returns (gh_in, ge_in, [grads dict per layer])."""
    real_w = H if ln_width is None else int(ln_width)
    grads = [None] * num_layers
    for i in reversed(range(num_layers)):
        if ss.dropout is not None:      # the gradient of layer i's output through layer i's mask (the caller's gh: out of place)
            gh = node_dropout(gh, ss.dropout, i, real_w, idx.get("nperm"), out=torch.empty_like(gh) if i == num_layers - 1 else None)
        gh, ge, grads[i] = layer_backward(idx, N, E, H, layer_params(P, i), ss.layers[i], gh, ge, batch_norm, ln_width=ln_width)
        ss.layers[i] = None
    return gh, ge, grads


@on_device_of(lambda scores, *a, **k: scores)
def bce_with_logits(scores, y, pos_weight: float):
    """(loss [1], dloss/dscores [E,1]) -- train.py:210-211,253-255, fused in one pass."""
    lib = _lib.load()
    _chk_dev(scores, y)
    x = _f32c(scores.reshape(-1))
    y = _f32c(y.reshape(-1))
    E = x.numel()
    sc = scratch(x.device)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    gs = torch.empty(E, 1, dtype=torch.float32, device=x.device)
    _call("gnm_bce_fwd_bwd", E, _ptr(x), _ptr(y), float(pos_weight), _ptr(loss), _ptr(gs),
                                   _ptr(sc.partials), sc.partials.numel() * 8, _stream())
    return loss, gs


@on_device_of(lambda scores, *a, **k: scores)
def bce_with_logits_counts(scores, y, pos_weight: float, need_grad: bool = True, epoch_acc=None):
    """(loss [1], dloss/dscores [E,1] or None, counts int64 [4] = TP TN FP FN) from one pass (gnm_bce_stats_fwd_bwd): the loss and
    the gradient are bce_with_logits' bit for bit.  need_grad=False stores no per-edge output.  epoch_acc: 48-byte device records
    ({double loss_sum; int64 steps; int64 counts[4]} as int64 [6] tensors, train.EpochStats.buf) that the step is added to."""
    lib = _lib.load()
    _chk_dev(scores, y)
    x = _f32c(scores.reshape(-1))
    y = _f32c(y.reshape(-1))
    E = x.numel()
    sc = scratch(x.device)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    gs = torch.empty(E, 1, dtype=torch.float32, device=x.device) if need_grad else None
    counts = torch.empty(4, dtype=torch.int64, device=x.device)
    _chk_epoch_acc(scores, epoch_acc)
    _call("gnm_bce_stats_fwd_bwd", E, _ptr(x), _ptr(y), float(pos_weight), _ptr(loss), _ptr(gs), _ptr(counts), _ptr(epoch_acc),
          _ptr(sc.partials), sc.partials.numel() * 8, _stream())
    return loss, gs, counts


@on_device_of(lambda org, *a, **k: org)
def sym_bce(org, rev, y, pos_weight: float, alpha: float, need_grad: bool = True, want_counts: bool = False, epoch_acc=None):
    """The symmetry loss of one graph from one pass over the original and the reversed scores (gnm_sym_bce_fwd_bwd):
    (loss [1], parts [3] = mean bce(org), mean bce(rev), mean |org - rev|, g_org [E] or None, g_rev [E] or None, counts int64 [4]
    of org or None).  need_grad=False stores no per-edge output.  epoch_acc: as for bce_with_logits_counts."""
    lib = _lib.load()
    _chk_dev(org, rev, y)
    o = _f32c(org.reshape(-1))
    r = _f32c(rev.reshape(-1))
    y = _f32c(y.reshape(-1))
    E = o.numel()
    if r.numel() != E or y.numel() != E:
        raise ValueError(f"sym_bce: {E} original scores, {r.numel()} reversed scores, {y.numel()} labels")
    dev = o.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    parts = torch.empty(3, dtype=torch.float32, device=dev)
    go = torch.empty(E, dtype=torch.float32, device=dev) if need_grad else None
    gr = torch.empty(E, dtype=torch.float32, device=dev) if need_grad else None
    counts = torch.empty(4, dtype=torch.int64, device=dev) if want_counts else None
    _chk_epoch_acc(org, epoch_acc)
    need = lib.gnm_sym_bce_workspace_bytes()
    ws = scratch(dev).ws(need)
    _call("gnm_sym_bce_fwd_bwd", E, _ptr(o), _ptr(r), _ptr(y), float(pos_weight), float(alpha), _ptr(loss), _ptr(parts), _ptr(go),
          _ptr(gr), _ptr(counts), _ptr(epoch_acc), _ptr(ws), need, _stream())
    return loss, parts, go, gr, counts


@on_device_of(lambda g, *a, **k: g)
def mirror_add(g, scratch_grad, pi):
    """g[i] += scratch_grad[pi[i]] over flat fp32 buffers (gnm_mirror_add, one launch): the gradient of a pass that ran on the
    mirrored parameters flat[pi], folded into the flat gradient buffer.  pi: int32 permutation (models.mirror_index)."""
    _chk_dev(g, scratch_grad, pi)
    n = g.numel()
    if not (_fits(g, torch.float32, n) and _fits(scratch_grad, torch.float32, n) and _fits(pi, torch.int32, n)):
        raise ValueError(f"mirror_add: contiguous float32 buffers and an int32 permutation of {n} elements each")
    _call("gnm_mirror_add", n, _ptr(g), _ptr(scratch_grad), _ptr(pi), _stream())
    return g


@on_device_of(lambda src, *a, **k: src)
def mirror_gather(src, pi, out=None):
    """out[i] = src[pi[i]] over flat fp32 buffers (gnm_mirror_gather, one launch): the mirrored copy of a flat parameter buffer."""
    _chk_dev(src, pi, out)
    n = src.numel()
    if out is None:
        out = torch.empty_like(src)
    if not (_fits(src, torch.float32, n) and _fits(out, torch.float32, n) and _fits(pi, torch.int32, n)
            and out.data_ptr() != src.data_ptr()):
        raise ValueError(f"mirror_gather: contiguous float32 buffers (out is not src) and an int32 permutation of {n} elements each")
    _call("gnm_mirror_gather", n, _ptr(out), _ptr(src), _ptr(pi), _stream())
    return out


RANK_BINS = 16384                      # bins per label of a gnm_rank_record (include/gnm.h): the 14-bit key of an fp32 logit
RANK_RECORD_WORDS = 2 * RANK_BINS + 4  # int64 hist[2][RANK_BINS], then tail[4] = nan_pos, nan_neg, other_label, calls


@on_device_of(lambda scores, *a, **k: scores)
def rank_hist(scores, y, record):
    """Add the (score, label) pairs to `record` (gnm_rank_hist, one launch on the current stream): a contiguous int64
    [RANK_RECORD_WORDS] device tensor holding a gnm_rank_record (train.RankingStats.buf), which the caller zeroes once."""
    lib = _lib.load()
    _chk_dev(scores, y, record)
    x, y, E = _scores_labels("rank_hist", scores, y)
    _chk_record("rank_hist", record, RANK_RECORD_WORDS, owner=" (train.RankingStats.buf)")
    need = lib.gnm_rank_hist_workspace_bytes(E)
    ws = scratch(x.device).ws(need) if need else None
    _call("gnm_rank_hist", E, _ptr(x), _ptr(y), _ptr(record), _ptr(ws), need, _stream())


DECISION_COUNTERS = ("dead", "forced", "forced_ok", "branch", "branch_solvable", "branch_ok", "branch_nan")
DECISION_RECORD_WORDS = 2 * len(DECISION_COUNTERS) + 1   # int64 dir[2][7] (successors, predecessors), then calls (include/gnm.h)
_DECISION_INDEX_KEYS = ("perm", "isrc", "idst", "in_ptr", "out_ptr", "out_pos", "out_dst")


@on_device_of(lambda idx, scores, y, record, *a, **k: record)
def decision_stats(idx, scores, y, record, best_succ=None, best_pred=None):
    """Add the walk decisions of one graph to `record` (gnm_decision_stats, one launch on the current stream): per node the
    top-scored out-edge and in-edge, self loops left out, ties to the lowest edge id, NaN below every number.
    idx: the graph's index (dict of graph.index(device)); scores [E] in edge-id order; y [E] labels or None (then only dead,
    forced, branch and branch_nan move); record: a contiguous int64 [DECISION_RECORD_WORDS] device tensor
    (train.DecisionStats.buf), which the caller zeroes once; best_succ / best_pred: None, or contiguous int32 [n] tensors that
    receive the chosen edge ids in the CALLER's node numbering (-1: no candidate)."""
    n = int(idx["in_ptr"].numel()) - 1
    nperm = idx.get("nperm")
    _chk_dev(scores, y, record, best_succ, best_pred, nperm, *[idx[k] for k in _DECISION_INDEX_KEYS])
    if scores.numel() != idx["perm"].numel():
        raise ValueError(f"decision_stats: {scores.numel()} scores for an index of {idx['perm'].numel()} edges")
    x, y, E = _scores_labels("decision_stats", scores, y)
    _chk_record("decision_stats", record, DECISION_RECORD_WORDS, owner=" (train.DecisionStats.buf)")
    _chk_args("decision_stats", ("best_succ", best_succ, torch.int32, n), ("best_pred", best_pred, torch.int32, n),
              optional=("best_succ", "best_pred"))
    _chk_index("decision_stats", idx, _DECISION_INDEX_KEYS, n)
    _call("gnm_decision_stats", n, E, _ptr(idx["perm"]), _ptr(idx["isrc"]), _ptr(idx["idst"]), _ptr(idx["in_ptr"]), _ptr(idx["out_ptr"]),
          _ptr(idx["out_pos"]), _ptr(idx["out_dst"]), _ptr(nperm), _ptr(x), _ptr(y), _ptr(record), _ptr(best_succ), _ptr(best_pred),
          _stream())


class RecordStats:
    """Base of the dataclasses that hold one device record of counters on the host (decode.BogStats, ReduceStats, SeqStats,
    features.AlignStats): the fields are the record's int64 words in order, the names of the record's *_COUNTERS tuple below."""

    @classmethod
    def from_record(cls, rec: torch.Tensor):
        """The record tensor as a stats object: one device-to-host copy, which synchronises."""
        return cls(*[int(v) for v in rec.cpu().tolist()])

    def words(self) -> List[int]:
        return [getattr(self, f.name) for f in fields(self)]


BOG_COUNTERS = ("contigs", "links", "cycles_cut", "dropped", "wrong_links", "multi_nodes", "multi_contigs", "calls")
BOG_RECORD_WORDS = len(BOG_COUNTERS)       # the int64 words of a gnm_bog_record (include/gnm.h), in order


@on_device_of(lambda src, dst, best_succ, best_pred, scores, y, prefix_length, read_length, record, *a, **k: record)
def bog_contigs(src, dst, best_succ, best_pred, scores, y, prefix_length, read_length, record, contig_ptr, walk_nodes, walk_edges,
                contig_bases, contig_wrong, min_logit: float = float("-inf")):
    """The best-overlap contigs of one graph (gnm_bog_contigs: 2 ceil(log2 n) + 6 launches on the current stream, no host
    synchronisation): the edges that are the best successor of their source and the best predecessor of their destination, cycles
    cut at their smallest node, the resulting paths ranked and laid out.  Caller's node numbering, edge-id order.
    src, dst [E] int32; best_succ, best_pred [n] int32 (decision_stats); scores [E]; y [E] labels or None; prefix_length [E] and
    read_length [n] int64; record: a contiguous int64 [BOG_RECORD_WORDS] device tensor the call ADDS to (the caller zeroes it and
    reads the contig count C from it); contig_ptr int32 [n+1]; walk_nodes, walk_edges, contig_wrong int32 [n]; contig_bases int64
    [n] -- of contig_ptr / contig_bases / contig_wrong only the first C+1 / C / C entries are defined."""
    lib = _lib.load()
    _chk_dev(src, dst, best_succ, best_pred, scores, y, prefix_length, read_length, record, contig_ptr, walk_nodes, walk_edges,
             contig_bases, contig_wrong)
    n, E = int(best_succ.numel()), int(src.numel())
    if scores.numel() != E or dst.numel() != E:
        raise ValueError(f"bog_contigs: {E} src entries, {dst.numel()} dst entries, {scores.numel()} scores")
    x, y, _ = _scores_labels("bog_contigs", scores, y)
    _chk_record("bog_contigs", record, BOG_RECORD_WORDS)
    _chk_args("bog_contigs", ("src", src, torch.int32, E), ("dst", dst, torch.int32, E), ("best_succ", best_succ, torch.int32, n),
              ("best_pred", best_pred, torch.int32, n), ("prefix_length", prefix_length, torch.int64, E),
              ("read_length", read_length, torch.int64, n), ("contig_ptr", contig_ptr, torch.int32, n + 1),
              ("walk_nodes", walk_nodes, torch.int32, n), ("walk_edges", walk_edges, torch.int32, n),
              ("contig_bases", contig_bases, torch.int64, n), ("contig_wrong", contig_wrong, torch.int32, n))
    need = lib.gnm_bog_workspace_bytes(n)
    ws = scratch(record.device).ws(need) if need else None
    _call("gnm_bog_contigs", n, E, _ptr(src), _ptr(dst), _ptr(best_succ), _ptr(best_pred), _ptr(x), _ptr(y), _ptr(prefix_length),
          _ptr(read_length), float(min_logit), _ptr(record), _ptr(contig_ptr), _ptr(walk_nodes), _ptr(walk_edges), _ptr(contig_bases),
          _ptr(contig_wrong), _ptr(ws), need, _stream())


_COVER_INDEX_KEYS = ("perm", "isrc", "in_ptr", "out_ptr", "out_pos", "out_dst")


@on_device_of(lambda idx, scores, round_links, *a, **k: round_links)
def cover_rounds(idx, scores, round_links, link_succ, link_pred, ws, first_round: int = 0, min_logit: float = float("-inf")):
    """Rounds first_round .. first_round + len(round_links) - 1 of the greedy path cover (gnm_cover_rounds: two launches per round
    and two per call on the current stream, no host synchronisation): every node with a free out- / in-slot proposes its best
    candidate edge whose other end is free, and an edge both ends proposed becomes a link.  first_round == 0 starts from the empty
    cover; a later call continues on `ws`, which the caller keeps and leaves untouched in between.
    idx: the graph's index (dict of graph.index(device)); scores [E] in edge-id order; round_links: a contiguous int64 [rounds]
    device tensor that receives the links every round of this call added; link_succ / link_pred: contiguous int32 [n] tensors that
    receive the cover so far in the CALLER's node numbering (edge ids, -1: the slot is free) -- what bog_contigs takes as best_succ
    / best_pred; ws: a contiguous uint8 tensor of at least cover_workspace_bytes(n) bytes (the state between calls)."""
    lib = _lib.load()
    n = int(idx["in_ptr"].numel()) - 1
    nperm = idx.get("nperm")
    _chk_dev(scores, round_links, link_succ, link_pred, ws, nperm, *[idx[k] for k in _COVER_INDEX_KEYS])
    if scores.numel() != idx["perm"].numel():
        raise ValueError(f"cover_rounds: {scores.numel()} scores for an index of {idx['perm'].numel()} edges")
    x, _, E = _scores_labels("cover_rounds", scores, None)
    if round_links.dtype != torch.int64 or round_links.dim() != 1 or not round_links.is_contiguous():
        raise ValueError("cover_rounds: round_links must be a contiguous int64 [rounds] tensor")
    if int(first_round) < 0:
        raise ValueError(f"cover_rounds: first_round = {first_round}: expected >= 0")
    _chk_args("cover_rounds", ("link_succ", link_succ, torch.int32, n), ("link_pred", link_pred, torch.int32, n))
    _chk_index("cover_rounds", idx, _COVER_INDEX_KEYS, n)
    need = lib.gnm_cover_workspace_bytes(n)
    if ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous():
        raise ValueError(f"cover_rounds: ws must be a contiguous uint8 tensor of at least {need} bytes (cover_workspace_bytes)")
    _call("gnm_cover_rounds", n, E, _ptr(idx["perm"]), _ptr(idx["isrc"]), _ptr(idx["in_ptr"]), _ptr(idx["out_ptr"]), _ptr(idx["out_pos"]),
          _ptr(idx["out_dst"]), _ptr(nperm), _ptr(x), float(min_logit), int(first_round), int(round_links.numel()), _ptr(round_links),
          _ptr(link_succ), _ptr(link_pred), _ptr(ws), int(ws.numel()), _stream())


def cover_workspace_bytes(n: int) -> int:
    """gnm_cover_workspace_bytes: the bytes of state cover_rounds keeps per graph of n nodes between its calls."""
    return int(_lib.load().gnm_cover_workspace_bytes(int(n)))


RESOLVE_COUNTERS = ("contigs", "eligible", "pieces", "dropped", "nodes", "serial", "invalid", "calls")
RESOLVE_RECORD_WORDS = len(RESOLVE_COUNTERS)  # the int64 words of a gnm_resolve_record (include/gnm.h), in order


def resolve_workspace_bytes(C: int, P: int, n: int) -> int:
    """gnm_resolve_workspace_bytes: the bytes of state the three resolve_* calls share for C contigs of P positions over n nodes."""
    return int(_lib.load().gnm_resolve_workspace_bytes(int(C), int(P), int(n)))


def _resolve_head(fn: str, cover, n: int, E: int, len_threshold: int, record, ws, *more):
    """The arguments the three resolve_* wrappers share, checked: cover = (contig_ptr [C+1], walk_nodes [P], walk_edges [P], order
    [C]) int32; returns the leading arguments of the entry point and the trailing (ws, bytes, stream)."""
    contig_ptr, walk_nodes, walk_edges, order = cover
    _chk_dev(contig_ptr, walk_nodes, walk_edges, order, record, ws, *more)
    nc, P = int(contig_ptr.numel()) - 1, int(walk_nodes.numel())
    if nc < 0:
        raise ValueError(f"{fn}: contig_ptr is empty: expected C + 1 entries, at least the leading 0")
    if isinstance(len_threshold, bool) or not hasattr(len_threshold, "__index__") or operator.index(len_threshold) < 1:
        raise ValueError(f"{fn}: len_threshold={len_threshold!r}: expected an integer >= 1")
    _chk_record(fn, record, RESOLVE_RECORD_WORDS)
    _chk_args(fn, ("contig_ptr", contig_ptr, torch.int32, nc + 1), ("walk_nodes", walk_nodes, torch.int32, P),
              ("walk_edges", walk_edges, torch.int32, P), ("order", order, torch.int32, nc))
    need = resolve_workspace_bytes(nc, P, n)
    if ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous():
        raise ValueError(f"{fn}: ws must be a contiguous uint8 tensor of at least {need} bytes (resolve_workspace_bytes)")
    head = (nc, P, int(n), int(E), _ptr(contig_ptr), _ptr(walk_nodes), _ptr(walk_edges), _ptr(order), operator.index(len_threshold))
    return head, (_ptr(ws), int(ws.numel()), _stream())


@on_device_of(lambda cover, n, E, len_threshold, record, ws: record)
def resolve_prepare(cover, n, E, len_threshold, record, ws):
    """Reset `ws`, check the cover and classify its contigs (gnm_resolve_prepare: 3 launches, no host synchronisation).  cover:
    (contig_ptr, walk_nodes, walk_edges, order) contiguous int32 device tensors -- a BogContigs' CSR and the contigs in priority
    order; n nodes, E edges; record: a contiguous int64 [RESOLVE_RECORD_WORDS] device tensor the call ADDS to; ws: a contiguous
    uint8 tensor of at least resolve_workspace_bytes(C, P, n) bytes, kept for resolve_rounds and resolve_layout."""
    head, tail = _resolve_head("resolve_prepare", cover, n, E, len_threshold, record, ws)
    _call("gnm_resolve_prepare", *head, _ptr(record), *tail)


@on_device_of(lambda cover, n, E, len_threshold, undecided, *a, **k: undecided)
def resolve_rounds(cover, n, E, len_threshold, undecided, record, ws, first_round: int = 0):
    """Rounds first_round .. first_round + len(undecided) - 1 of the strand rule on the state resolve_prepare left in `ws`
    (gnm_resolve_rounds: one launch per round and one per call): undecided, a contiguous int64 [rounds] device tensor, receives
    the contigs not finished after every round, -1 when resolve_prepare found the input invalid."""
    if undecided.dtype != torch.int64 or undecided.dim() != 1 or not undecided.is_contiguous():
        raise ValueError("resolve_rounds: undecided must be a contiguous int64 [rounds] tensor")
    if int(first_round) < 0:
        raise ValueError(f"resolve_rounds: first_round = {first_round}: expected >= 0")
    head, tail = _resolve_head("resolve_rounds", cover, n, E, len_threshold, record, ws, undecided)
    _call("gnm_resolve_rounds", *head, int(first_round), int(undecided.numel()), _ptr(undecided), _ptr(record), *tail)


@on_device_of(lambda cover, n, E, len_threshold, prefix_length, read_length, y, record, *a, **k: record)
def resolve_layout(cover, n, E, len_threshold, prefix_length, read_length, y, record, out_ptr, out_nodes, out_edges, out_bases,
                   out_wrong, ws):
    """The kept pieces of a finished resolve_rounds state as a cover of their own (gnm_resolve_layout: 5 launches, no host
    synchronisation): out_ptr int32 [P+1], out_nodes, out_edges, out_wrong int32 [P], out_bases int64 [P], of which the first
    K+1 / N / N / K / K entries are defined (record.pieces, record.nodes).  prefix_length [E], read_length [n] int64; y [E] labels
    or None."""
    P = int(cover[1].numel())
    if y is not None:
        y = _f32c(y.reshape(-1).float())
    head, tail = _resolve_head("resolve_layout", cover, n, E, len_threshold, record, ws, prefix_length, read_length, y, out_ptr,
                               out_nodes, out_edges, out_bases, out_wrong)
    _chk_args("resolve_layout", ("prefix_length", prefix_length, torch.int64, int(E)), ("read_length", read_length, torch.int64, int(n)),
              ("y", y, torch.float32, int(E)), ("out_ptr", out_ptr, torch.int32, P + 1), ("out_nodes", out_nodes, torch.int32, P),
              ("out_edges", out_edges, torch.int32, P), ("out_bases", out_bases, torch.int64, P),
              ("out_wrong", out_wrong, torch.int32, P), optional=("y",))
    _call("gnm_resolve_layout", *head, _ptr(prefix_length), _ptr(read_length), _ptr(y), _ptr(record), _ptr(out_ptr), _ptr(out_nodes),
          _ptr(out_edges), _ptr(out_bases), _ptr(out_wrong), *tail)


REDUCE_COUNTERS = ("edges", "candidates", "reduced", "reduced_label1", "witnesses", "max_support", "self_loops", "calls")
REDUCE_RECORD_WORDS = len(REDUCE_COUNTERS)  # the int64 words of a gnm_reduce_record (include/gnm.h), in order


def reduce_fuzz_word(fuzz, what: str = "fuzz") -> int:
    """The `fuzz` argument of gnm_transitive_support for a Python value: -1 for None (no length test), else the integer, which
    must be >= 0 (a bool is refused: it is no length); `what` names the argument in the ValueError."""
    if fuzz is None:
        return -1
    ok = not isinstance(fuzz, bool) and type(fuzz).__name__ != "bool_" and hasattr(fuzz, "__index__")
    if not ok or not 0 <= operator.index(fuzz) < 2 ** 63:
        raise ValueError(f"{what}={fuzz!r}: expected None or an integer >= 0")
    return operator.index(fuzz)


@on_device_of(lambda idx, scores, prefix_length, y, min_logit, fuzz, support, masked_scores, rec: rec)
def transitive_support(idx, scores, prefix_length, y, min_logit, fuzz, support, masked_scores, rec):
    """The transitive support of every edge (gnm_transitive_support: one launch on the current stream, no workspace, no host
    synchronisation): for k = (a -> c) the number of candidate out-edges a -> b of strictly smaller prefix that a candidate b -> c
    closes -- within `fuzz` bases of prefix_length[k], or at all when fuzz is None / -1.  A candidate is cover_rounds': no self
    loop, no NaN, scores >= min_logit.
    idx: the graph's index (dict of graph.index(device)); scores [E], prefix_length [E] int64 and y [E] labels or None in edge-id
    order; support: a contiguous int32 [E] tensor; masked_scores: None, or a contiguous fp32 [E] tensor (not `scores` itself) that
    receives the scores with a NaN on every reduced edge (a candidate with support > 0) -- what decision_stats, cover_rounds and
    bog_contigs take in place of the scores; rec: a contiguous int64 [REDUCE_RECORD_WORDS] device tensor the call ADDS to (the
    caller zeroes it once).  A graph without an edge launches nothing and leaves rec as it is."""
    n = int(idx["in_ptr"].numel()) - 1
    nperm = idx.get("nperm")
    _chk_dev(scores, prefix_length, y, support, masked_scores, rec, nperm, *[idx[k] for k in _COVER_INDEX_KEYS])
    if scores.numel() != idx["perm"].numel():
        raise ValueError(f"transitive_support: {scores.numel()} scores for an index of {idx['perm'].numel()} edges")
    x, y, E = _scores_labels("transitive_support", scores, y)
    fz = reduce_fuzz_word(fuzz, "transitive_support: fuzz")
    _chk_record("transitive_support", rec, REDUCE_RECORD_WORDS, "rec")
    _chk_args("transitive_support", ("prefix_length", prefix_length, torch.int64, E), ("support", support, torch.int32, E),
              ("masked_scores", masked_scores, torch.float32, E), optional=("masked_scores",))
    if masked_scores is not None and E and masked_scores.data_ptr() == x.data_ptr():
        raise ValueError("transitive_support: masked_scores must not be the scores tensor itself (a witness reads the scores)")
    _chk_index("transitive_support", idx, _COVER_INDEX_KEYS, n)
    _call("gnm_transitive_support", n, E, _ptr(idx["perm"]), _ptr(idx["isrc"]), _ptr(idx["in_ptr"]), _ptr(idx["out_ptr"]),
          _ptr(idx["out_pos"]), _ptr(idx["out_dst"]), _ptr(nperm), _ptr(x), _ptr(prefix_length), _ptr(y), float(min_logit), int(fz),
          _ptr(support), _ptr(masked_scores), _ptr(rec), _stream())


SEQ_COUNTERS = ("contigs", "pieces", "bases", "clamped", "empty", "reverse", "invalid", "calls")
SEQ_RECORD_WORDS = len(SEQ_COUNTERS)       # the int64 words of a gnm_seq_record (include/gnm.h), in order
SEQ_CHUNK_BASES = 4096                     # GNM_SEQ_CHUNK_BASES: output bases a workgroup of gnm_seq_emit owns at a time
SEQ_LETTERS = "=ACMGRSVTWYHKDBN"           # the letter of every 4-bit code


def _seq_store_args(name, base_off, length, packed):
    R = int(base_off.numel())
    _chk_args(name, ("base_off", base_off, torch.int64, R), ("length", length, torch.int64, R),
              ("packed", packed, torch.uint8, packed.numel()))
    if packed.numel() % 16:
        raise ValueError(f"{name}: packed holds {packed.numel()} bytes, not whole 16-byte groups")
    return R


@on_device_of(lambda contig_ptr, *a, **k: contig_ptr)
def seq_layout(contig_ptr, walk_nodes, walk_edges, prefix_length, n: int, base_off, length, packed, record, piece_len, piece_off,
               contig_base_ptr):
    """Piece lengths, their exclusive prefix sum and the contigs' base offsets for walks in CSR form over a packed read store
    (gnm_seq_layout: 4 launches on the current stream, no host synchronisation).  contig_ptr int32 [C+1]; walk_nodes, walk_edges
    int32 [P]; prefix_length int64 [E]; n: nodes of the graph; base_off, length int64 [R] and packed uint8 (whole 16-byte groups):
    the store; record: a contiguous int64 [SEQ_RECORD_WORDS] device tensor the call ADDS to; piece_len int64 [P], piece_off int64
    [P+1], contig_base_ptr int64 [C+1]: outputs."""
    lib = _lib.load()
    _chk_dev(contig_ptr, walk_nodes, walk_edges, prefix_length, base_off, length, packed, record, piece_len, piece_off, contig_base_ptr)
    C, P, E = int(contig_ptr.numel()) - 1, int(walk_nodes.numel()), int(prefix_length.numel())
    if C < 0:
        raise ValueError("seq_layout: contig_ptr needs at least one entry")
    R = _seq_store_args("seq_layout", base_off, length, packed)
    _chk_record("seq_layout", record, SEQ_RECORD_WORDS)
    _chk_args("seq_layout", ("contig_ptr", contig_ptr, torch.int32, C + 1), ("walk_nodes", walk_nodes, torch.int32, P),
              ("walk_edges", walk_edges, torch.int32, P), ("prefix_length", prefix_length, torch.int64, E),
              ("piece_len", piece_len, torch.int64, P), ("piece_off", piece_off, torch.int64, P + 1),
              ("contig_base_ptr", contig_base_ptr, torch.int64, C + 1))
    need = lib.gnm_seq_workspace_bytes(P)
    ws = scratch(record.device).ws(need) if need else None
    _call("gnm_seq_layout", C, P, E, int(n), R, _ptr(contig_ptr), _ptr(walk_nodes), _ptr(walk_edges), _ptr(prefix_length),
          _ptr(base_off), _ptr(length), int(packed.numel()), _ptr(record), _ptr(piece_len), _ptr(piece_off), _ptr(contig_base_ptr),
          _ptr(ws), need, _stream())


@on_device_of(lambda walk_nodes, piece_off, *a, **k: piece_off)
def seq_emit(walk_nodes, piece_off, n: int, base_off, length, packed, total: int, out):
    """The bases of the laid-out pieces as ASCII (gnm_seq_emit: one launch, none when total == 0).  walk_nodes int32 [P] and
    piece_off int64 [P+1] as seq_layout left them; total: record.bases of that call; out: uint8, a multiple of 16 bytes >= total.
    Bytes [0, total) are written, and the rest of the last 16-byte group as 0."""
    _lib.load()
    _chk_dev(walk_nodes, piece_off, base_off, length, packed, out)
    P = int(walk_nodes.numel())
    R = _seq_store_args("seq_emit", base_off, length, packed)
    _chk_args("seq_emit", ("walk_nodes", walk_nodes, torch.int32, P), ("piece_off", piece_off, torch.int64, P + 1),
              ("out", out, torch.uint8, out.numel()))
    _call("gnm_seq_emit", P, int(n), R, _ptr(walk_nodes), _ptr(piece_off), _ptr(base_off), _ptr(length), _ptr(packed),
          int(packed.numel()), int(total), _ptr(out), int(out.numel()), _stream())


ALIGN_COUNTERS = ("edges", "aligned", "exceeded", "empty", "clamped", "invalid", "cells", "calls")
ALIGN_RECORD_WORDS = len(ALIGN_COUNTERS)   # the int64 words of a gnm_align_record (include/gnm.h), in order
ALIGN_MAX_ERRORS = 255                     # the widest band: 2 K + 1 <= 512 diagonals


def _align_args(name, src, dst, prefix_length, base_off, length, packed, max_errors, dist, overlap_length, similarity, rec):
    E = int(src.numel())
    R = _seq_store_args(name, base_off, length, packed)
    _int_in(name, "max_errors", max_errors, 0, ALIGN_MAX_ERRORS)
    _chk_record(name, rec, ALIGN_RECORD_WORDS, "rec")
    _chk_args(name, ("src", src, torch.int32, E), ("dst", dst, torch.int32, E), ("prefix_length", prefix_length, torch.int64, E),
              ("dist", dist, torch.int32, E), ("overlap_length", overlap_length, torch.int64, E),
              ("similarity", similarity, torch.float32, E))
    return E, R


@on_device_of(lambda src, *a, **k: src)
def overlap_align(src, dst, prefix_length, n: int, base_off, length, packed, max_errors: int, dist, overlap_length, similarity, rec):
    """The banded edit distance of every edge's overlap (gnm_overlap_align: one launch on the current stream, no workspace, no
    host synchronisation; none at all for E == 0).  src, dst int32 [E] and prefix_length int64 [E] in edge-id order; n: nodes of
    the graph; base_off, length int64 [R] and packed uint8 (whole 16-byte groups): the read store; max_errors: the K of the rule,
    0 .. ALIGN_MAX_ERRORS; dist int32 [E] (K + 1: exceeded, -1: invalid), overlap_length int64 [E], similarity fp32 [E]: outputs;
    rec: a contiguous int64 [ALIGN_RECORD_WORDS] device tensor the call ADDS to (the caller zeroes it once)."""
    _lib.load()
    _chk_dev(src, dst, prefix_length, base_off, length, packed, dist, overlap_length, similarity, rec)
    E, R = _align_args("overlap_align", src, dst, prefix_length, base_off, length, packed, max_errors, dist, overlap_length,
                       similarity, rec)
    _call("gnm_overlap_align", E, _ptr(src), _ptr(dst), _ptr(prefix_length), _ptr(packed), int(packed.numel()), _ptr(base_off),
          _ptr(length), R, int(n), operator.index(max_errors), _ptr(dist), _ptr(overlap_length), _ptr(similarity), _ptr(rec), _stream())


def overlap_align_host(src, dst, prefix_length, n: int, base_off, length, packed, max_errors: int, dist, overlap_length, similarity,
                       rec, threads: int = 1):
    """overlap_align's arithmetic on the CPU (gnm_overlap_align_host: the same header routine, `threads` host threads): the same
    arguments as CPU tensors.  For tests and for scale; nothing on the product path calls it."""
    lib = _lib.load()
    _cpu_tensors("overlap_align_host", src, dst, prefix_length, base_off, length, packed, dist, overlap_length, similarity, rec)
    E, R = _align_args("overlap_align_host", src, dst, prefix_length, base_off, length, packed, max_errors, dist, overlap_length,
                       similarity, rec)
    _lib.check(lib.gnm_overlap_align_host(E, _hp(src), _hp(dst), _hp(prefix_length), _hp(packed), int(packed.numel()), _hp(base_off),
                                          _hp(length), R, int(n), operator.index(max_errors), _hp(dist), _hp(overlap_length),
                                          _hp(similarity), _hp(rec), int(threads)), "gnm_overlap_align_host")


OVERLAP_COUNTERS = ("reads", "kmers_valid", "minimizers", "runs", "skipped_runs", "skipped_entries", "hits", "same_read", "groups",
                    "few_hits", "short", "contained_groups", "links", "calls")
OVERLAP_RECORD_WORDS = len(OVERLAP_COUNTERS)   # the int64 words of a gnm_overlap_record (include/gnm.h), in order (`short`: too_short)
SKETCH_TILE = 512                              # GNM_SKETCH_TILE: k-mer positions one workgroup of the sketch kernels owns at a time
SKETCH_K, SKETCH_W, OVERLAP_MAX_OCC = (8, 31), (1, 64), 4096


def _int_in(fn: str, name: str, v, lo: int, hi: int) -> int:
    """v as an int in [lo, hi]; a bool or a float is no count."""
    if isinstance(v, bool) or type(v).__name__ == "bool_" or not hasattr(v, "__index__") or not lo <= operator.index(v) <= hi:
        raise ValueError(f"{fn}: {name}={v!r}: expected an integer in [{lo}, {hi}]")
    return operator.index(v)


def _hp(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _cpu_tensors(fn: str, *ts):
    if any(t is not None and t.device.type != "cpu" for t in ts):
        raise ValueError(f"{fn}: every tensor must be a CPU tensor")


def _new(dev, n, dt):
    return torch.empty(int(n), dtype=dt, device=dev)


def _count_then_emit(fn: str, ts, rec, threads, head, outs, extra, table_sizes, count, emit):
    """What sketch, seed_pairs and chain_pairs share: the outputs outs(m) of a stage whose size m only its count pass knows.
    ts: the stage's tensors, the one that names its device first; head(p): the leading arguments of gnm_<fn>_host, pointers made
    by p; extra: tensors of the caller's that follow the outputs there.
    CPU tensors: gnm_<fn>_host with capacity -1 and nulls for the size, then again over the outputs.
    Device tensors: count(tables, ws, need) enqueues the count pass over int64 tables of table_sizes entries and the scan workspace
    of the longest; the scan's total is the last table's last entry: ONE read-back; emit(tables, out) enqueues the emit pass."""
    lib = _lib.load()
    dev = ts[0].device
    if dev.type == "cpu":
        _cpu_tensors(fn, *ts, rec)
        host, total = getattr(lib, f"gnm_{fn}_host"), C.c_int64(0)
        tail = (C.byref(total), _hp(rec), int(threads))
        _lib.check(host(*head(_hp), -1, *[None] * (len(outs(0)) + len(extra)), *tail), f"gnm_{fn}_host")
        out = outs(total.value)
        _lib.check(host(*head(_hp), total.value, *[C.c_void_p(t.data_ptr()) for t in out + extra], *tail), f"gnm_{fn}_host")
        return out
    _chk_dev(*ts, rec)
    with torch.cuda.device(dev):
        tables = [_new(dev, m, torch.int64) for m in table_sizes]
        need = lib.gnm_overlap_scan_workspace_bytes(max(table_sizes) - 1)
        count([_ptr(t) for t in tables], _ptr(scratch(dev).ws(need)), need)
        out = outs(int(tables[-1][-1]))                      # the scan's total: the one synchronisation of the stage
        emit([_ptr(t) for t in tables], out)
    return out


def sketch(base_off, length, packed, k: int, w: int, rec, threads: int = 1):
    """The minimizer sketch of every read of a packed store (include/gnm.h, "overlap graph", stage 1): (hash int64, read int32, pos
    int32, strand uint8), ordered by read and position, on the store's device.  Device tensors: gnm_sketch_count, one read-back of
    the size, gnm_sketch_emit.  CPU tensors: gnm_sketch_host on `threads` host threads (the same header).  rec: a contiguous int64
    [OVERLAP_RECORD_WORDS] tensor on that device the call ADDS to."""
    R = _seq_store_args("sketch", base_off, length, packed)
    k, w = _int_in("sketch", "k", k, *SKETCH_K), _int_in("sketch", "w", w, *SKETCH_W)
    _chk_record("sketch", rec, OVERLAP_RECORD_WORDS, "rec")
    dev, nbytes = packed.device, int(packed.numel())
    tb = int(_lib.load().gnm_sketch_tile_bound(R, nbytes))
    head = lambda p: (p(packed), nbytes, p(base_off), p(length), R, k, w)  # noqa: E731
    return _count_then_emit(
        "sketch", (packed, base_off, length), rec, threads, head,
        lambda m: tuple(_new(dev, m, dt) for dt in (torch.int64, torch.int32, torch.int32, torch.uint8)), (),
        (R + 1, tb + 1),                                     # tile_ptr, tile_off
        lambda tables, ws, need: _call("gnm_sketch_count", *head(_ptr), *tables, tb, _ptr(rec), ws, need, _stream()),
        lambda tables, out: _call("gnm_sketch_emit", *head(_ptr), *tables, tb, out[0].numel(), *map(_ptr, out), _stream()))


def seed_pairs(hash_, read, pos, strand, length, k: int, max_occ: int, rec, threads: int = 1):
    """The seed hits of a sketch sorted by hash (stage 2): (key int64, diag int32).  hash_ int64, read, pos int32, strand uint8 [M]
    sorted stably by hash_; length int64 [R]: the reads' lengths.  Device or CPU tensors, as for `sketch`."""
    M, R = int(hash_.numel()), int(length.numel())
    k, max_occ = _int_in("seed_pairs", "k", k, *SKETCH_K), _int_in("seed_pairs", "max_occ", max_occ, 1, OVERLAP_MAX_OCC)
    _chk_record("seed_pairs", rec, OVERLAP_RECORD_WORDS, "rec")
    _chk_args("seed_pairs", ("hash", hash_, torch.int64, M), ("read", read, torch.int32, M), ("pos", pos, torch.int32, M),
              ("strand", strand, torch.uint8, M), ("length", length, torch.int64, R))
    dev = hash_.device
    head = lambda p: (M, p(hash_), p(read), p(pos), p(strand), p(length), R, k, max_occ)  # noqa: E731
    return _count_then_emit(
        "seed_pairs", (hash_, read, pos, strand, length), rec, threads, head,
        lambda m: (_new(dev, m, torch.int64), _new(dev, m, torch.int32)), (),
        (M + 1,),                                            # off
        lambda off, ws, need: _call("gnm_seed_pairs_count", M, _ptr(hash_), _ptr(read), max_occ, *off, _ptr(rec), ws, need, _stream()),
        lambda off, out: _call("gnm_seed_pairs_emit", *head(_ptr), *off, out[0].numel(), *map(_ptr, out), _stream()))


def seed_pairs_lower_hits(hash_, read, R: int, max_occ: int, lower_hits, rec, threads: int = 1):
    """The plan of the chunked route (stage 2 in read-range chunks): lower_hits int64 [R], zeroed by the caller, receives per read
    the hits whose lower read id it is; rec is added to exactly as by seed_pairs' count pass.  hash_ int64, read int32 [M] sorted
    stably by hash_.  Device tensors: gnm_seed_pairs_lower_hits, one launch, no read-back.  CPU tensors: the host twin."""
    lib = _lib.load()
    M = int(hash_.numel())
    R, max_occ = _int_in("seed_pairs_lower_hits", "R", R, 0, 2 ** 31 - 2), _int_in("seed_pairs_lower_hits", "max_occ", max_occ, 1, OVERLAP_MAX_OCC)
    _chk_record("seed_pairs_lower_hits", rec, OVERLAP_RECORD_WORDS, "rec")
    _chk_args("seed_pairs_lower_hits", ("hash", hash_, torch.int64, M), ("read", read, torch.int32, M),
              ("lower_hits", lower_hits, torch.int64, R))
    dev = hash_.device
    if dev.type == "cpu":
        _cpu_tensors("seed_pairs_lower_hits", hash_, read, lower_hits, rec)
        _lib.check(lib.gnm_seed_pairs_lower_hits_host(M, _hp(hash_), _hp(read), max_occ, _hp(lower_hits), R, _hp(rec), int(threads)),
                   "gnm_seed_pairs_lower_hits_host")
        return lower_hits
    _chk_dev(hash_, read, lower_hits, rec)
    if any(t.device != dev for t in (read, lower_hits, rec)):
        raise ValueError("seed_pairs_lower_hits: every tensor must be on the device of hash")
    with torch.cuda.device(dev):
        _call("gnm_seed_pairs_lower_hits", M, _ptr(hash_), _ptr(read), max_occ, _ptr(lower_hits), R, _ptr(rec), None, 0, _stream())
    return lower_hits


def seed_pairs_range(hash_, read, pos, strand, length, k: int, max_occ: int, a_lo: int, a_hi: int, rec, threads: int = 1):
    """seed_pairs restricted to the hits whose lower read id lies in [a_lo, a_hi), 0 <= a_lo <= a_hi <= R, in seed_pairs' order:
    (key int64, diag int32).  rec is checked and left as it is (seed_pairs_lower_hits added the totals)."""
    M, R = int(hash_.numel()), int(length.numel())
    k, max_occ = _int_in("seed_pairs_range", "k", k, *SKETCH_K), _int_in("seed_pairs_range", "max_occ", max_occ, 1, OVERLAP_MAX_OCC)
    a_lo, a_hi = _int_in("seed_pairs_range", "a_lo", a_lo, 0, R), _int_in("seed_pairs_range", "a_hi", a_hi, 0, R)
    if a_lo > a_hi:
        raise ValueError(f"seed_pairs_range: a_lo={a_lo} > a_hi={a_hi}: expected 0 <= a_lo <= a_hi <= {R}")
    _chk_record("seed_pairs_range", rec, OVERLAP_RECORD_WORDS, "rec")
    _chk_args("seed_pairs_range", ("hash", hash_, torch.int64, M), ("read", read, torch.int32, M), ("pos", pos, torch.int32, M),
              ("strand", strand, torch.uint8, M), ("length", length, torch.int64, R))
    dev = hash_.device
    head = lambda p: (M, p(hash_), p(read), p(pos), p(strand), p(length), R, k, max_occ, a_lo, a_hi)  # noqa: E731
    return _count_then_emit(
        "seed_pairs_range", (hash_, read, pos, strand, length), rec, threads, head,
        lambda m: (_new(dev, m, torch.int64), _new(dev, m, torch.int32)), (),
        (M + 1,),                                            # off
        lambda off, ws, need: _call("gnm_seed_pairs_count_range", M, _ptr(hash_), _ptr(read), max_occ, a_lo, a_hi, R, *off, _ptr(rec), ws,
                                    need, _stream()),
        lambda off, out: _call("gnm_seed_pairs_emit_range", *head(_ptr), *off, out[0].numel(), *map(_ptr, out), _stream()))


def chain_pairs(key, diag, length, band: int, min_hits: int, min_overlap: int, rec, threads: int = 1):
    """The chains of the seed hits sorted by diag, then stably by key (stage 3): (src int32, dst int32, prefix_length int64,
    overlap_length int64, valid uint8) [2 G] -- group g owns slots 2g (the edge) and 2g + 1 (its twin) -- and contained uint8 [R]."""
    N, R = int(key.numel()), int(length.numel())
    band, min_hits = _int_in("chain_pairs", "band", band, 0, 2 ** 31 - 2), _int_in("chain_pairs", "min_hits", min_hits, 1, 2 ** 31 - 2)
    min_overlap = _int_in("chain_pairs", "min_overlap", min_overlap, 0, 2 ** 62)
    _chk_record("chain_pairs", rec, OVERLAP_RECORD_WORDS, "rec")
    _chk_args("chain_pairs", ("key", key, torch.int64, N), ("diag", diag, torch.int32, N), ("length", length, torch.int64, R))
    dev = key.device
    contained = torch.zeros(R, dtype=torch.uint8, device=dev)
    out = _count_then_emit(
        "chain_pairs", (key, diag, length), rec, threads,
        lambda p: (N, p(key), p(diag), p(length), R, band, min_hits, min_overlap),
        lambda g: tuple(_new(dev, 2 * g, dt) for dt in (torch.int32, torch.int32, torch.int64, torch.int64, torch.uint8)), (contained,),
        (N + 1,),                                            # off: the group number of every head
        lambda off, ws, need: _call("gnm_chain_count", N, _ptr(key), *off, _ptr(rec), ws, need, _stream()),
        lambda off, out: _call("gnm_chain_pairs", N, _ptr(key), _ptr(diag), *off, out[0].numel() // 2, _ptr(length), R, band, min_hits,
                               min_overlap, *map(_ptr, out), _ptr(contained), _ptr(rec), _stream()))
    return out + (contained,)


GT_COUNTERS = ("edges", "valid", "wrong_strand", "self_loops", "gap", "backward", "components", "singletons", "backbone", "positives",
               "twin_missing", "invalid", "calls")
GT_RECORD_WORDS = len(GT_COUNTERS)         # the int64 words of a gnm_gt_record (include/gnm.h), in order
GT_ROUNDS_PER_BATCH = 8                    # rounds enqueued per read-back of their `changed` words
_GT_INDEX_KEYS = ("perm", "isrc", "idst", "in_ptr", "out_ptr", "out_pos", "out_dst")
_GT_STAGES = ("components", "fwd", "bwd")


def gt_sweeps() -> int:
    """gnm_gt_sweeps: the sweeps a workgroup makes over its nodes per fwd / bwd round."""
    return int(_lib.load().gnm_gt_sweeps())


def _gt_args(fn, n, E, start, end, strand, twin, y, valid, backbone, component, top, rec):
    """The argument rules gt_labels and gt_labels_host share."""
    _chk_record(fn, rec, GT_RECORD_WORDS, "rec")
    _chk_args(fn, ("read_start", start, torch.int64, n), ("read_end", end, torch.int64, n), ("read_strand", strand, torch.int64, n),
              ("twin", twin, torch.int64, E), ("y", y, torch.float32, E), ("valid", valid, torch.uint8, E),
              ("backbone", backbone, torch.uint8, n), ("component", component, torch.int32, n), ("top", top, torch.int32, n),
              optional=("twin",))


_GT_INVALID = "every node needs 0 <= read_start < read_end < 2^32 and read_strand +1 or -1"


@on_device_of(lambda idx, src, dst, start, end, strand, twin, y, *a, **k: y)
def gt_labels(idx, src, dst, start, end, strand, twin, y, valid, backbone, component, top, rec, rounds_per_batch=None):
    """Ground-truth labels of one graph on the device (include/gnm.h, "ground-truth labels"): gnm_gt_prepare, then the three stages
    of gnm_gt_rounds in batches of `rounds_per_batch` rounds (default GT_ROUNDS_PER_BATCH) with one read-back of the batch's
    `changed` words each, then gnm_gt_emit.  idx: the graph's index (dict of graph.index(device)); src, dst int32 [E]: the caller's
    edge list (read only to check `twin`); start, end, strand int64 [n] in the caller's numbering; twin: None or int64 [E];
    y fp32 [E], valid uint8 [E], backbone uint8 [n], component, top int32 [n]: the outputs; rec: a contiguous int64
    [GT_RECORD_WORDS] device tensor the call ADDS to.  Returns the rounds every stage took, the confirming round included (they
    depend on the schedule; nothing else does).  Unusable node values raise ValueError before any output is written."""
    lib = _lib.load()
    n, E = int(idx["in_ptr"].numel()) - 1, int(idx["perm"].numel())
    nperm, nrank = idx.get("nperm"), idx.get("nrank")
    _chk_dev(src, dst, start, end, strand, twin, y, valid, backbone, component, top, rec, nperm, nrank, *[idx[k] for k in _GT_INDEX_KEYS])
    _gt_args("gt_labels", n, E, start, end, strand, twin, y, valid, backbone, component, top, rec)
    _chk_args("gt_labels", ("src", src, torch.int32, E), ("dst", dst, torch.int32, E), ("nrank", nrank, torch.int32, n),
              optional=("nrank",))
    _chk_index("gt_labels", idx, _GT_INDEX_KEYS, n)
    if (nperm is None) != (nrank is None):
        raise ValueError("gt_labels: the index carries nperm without nrank (graph.index())")
    batch = _int_in("gt_labels", "rounds_per_batch", GT_ROUNDS_PER_BATCH if rounds_per_batch is None else rounds_per_batch, 1, 4096)
    dev = y.device
    need = int(lib.gnm_gt_workspace_bytes(n, E))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    head = (n, E, *[_ptr(idx[k]) for k in _GT_INDEX_KEYS], _ptr(nperm), _ptr(nrank))
    tail = (_ptr(ws), need, _stream())
    _call("gnm_gt_prepare", *head, _ptr(start), _ptr(end), _ptr(strand), _ptr(rec), *tail)
    changed = torch.empty(batch, dtype=torch.int64, device=dev)
    rounds = {}
    for stage, name in enumerate(_GT_STAGES):
        done = 0
        while True:
            _call("gnm_gt_rounds", *head, stage, done, batch, _ptr(changed), *tail)
            got = changed.tolist()                           # the batch's one read-back
            if got[0] < 0:
                raise ValueError(f"gt_labels: {_GT_INVALID}")
            if 0 in got:
                done += got.index(0) + 1
                break
            done += batch
        rounds[name] = done
    _call("gnm_gt_emit", *head, _ptr(twin), _ptr(src), _ptr(dst), _ptr(y), _ptr(valid), _ptr(backbone), _ptr(component), _ptr(top),
          _ptr(rec), *tail)
    return rounds


def gt_labels_host(src, dst, n: int, start, end, strand, twin, y, valid, backbone, component, top, rec):
    """gt_labels on CPU tensors over the caller's edge list (gnm_gt_labels_host: the same header, union-find and queues; no index).
    Unusable node values raise ValueError and write nothing but rec's `invalid` word."""
    lib = _lib.load()
    n, E = int(n), int(src.numel())
    _cpu_tensors("gt_labels_host", src, dst, start, end, strand, twin, y, valid, backbone, component, top, rec)
    _gt_args("gt_labels_host", n, E, start, end, strand, twin, y, valid, backbone, component, top, rec)
    _chk_args("gt_labels_host", ("src", src, torch.int32, E), ("dst", dst, torch.int32, E))
    rc = lib.gnm_gt_labels_host(n, E, _hp(src), _hp(dst), _hp(start), _hp(end), _hp(strand), _hp(twin), _hp(y), _hp(valid),
                                _hp(backbone), _hp(component), _hp(top), _hp(rec))
    if rc != 0 and b"unusable" in lib.gnm_last_error():
        raise ValueError(f"gt_labels_host: {_GT_INVALID}, and every edge two nodes below n")
    _lib.check(rc, "gnm_gt_labels_host")
    return {name: 0 for name in _GT_STAGES}


def optim_workspace(n: int, device) -> torch.Tensor:
    """The workspace of optim_step for flat buffers of n elements (gnm_optim_workspace_bytes), as int64 words: 8-byte aligned."""
    return torch.empty((_lib.load().gnm_optim_workspace_bytes(int(n)) + 7) // 8, dtype=torch.int64, device=device)


@on_device_of(lambda p, *a, **k: p)
def optim_step(p, g, m, v, step, stats, ws, lr, beta1, beta2, eps, max_norm=0.0, inv_count=None, zero_grad=False):
    """One optimizer step over flat fp32 buffers, two launches on the current stream (gnm_optim_grad_stats, gnm_optim_adam_step;
    include/gnm.h): Adam with the gradient's norm clipped to max_norm (0: off), skipped as a whole when g holds a non-finite
    entry.  step: device float scalar; stats: int64 [4] holding a gnm_optim_stats; ws: optim_workspace(n)."""
    _chk_dev(p, g, m, v, step, stats, ws, inv_count)
    n = p.numel()
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        if not _fits(t, torch.float32, n):
            raise ValueError(f"optim_step: {name} must be a contiguous float32 tensor of {n} elements")
    if step.dtype != torch.float32 or step.numel() != 1 or (inv_count is not None and (inv_count.dtype != torch.float32 or inv_count.numel() != 1)):
        raise ValueError("optim_step: step (and inv_count) must be float32 scalars")
    _chk_record("optim_step", stats, 4, "stats")
    wsb = ws.numel() * ws.element_size()
    _call("gnm_optim_grad_stats", n, _ptr(g), _ptr(step), _ptr(ws), wsb, _stream())
    _call("gnm_optim_adam_step", n, _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(step), _ptr(stats), _ptr(ws), wsb, float(lr),
          float(beta1), float(beta2), float(eps), float(max_norm), _ptr(inv_count), int(bool(zero_grad)), _stream())


_default = Options(**{k: (globals()["_D_" + k] if k not in ("ACTIVATIONS", "TN_AT") else {"ACTIVATIONS": "saved", "TN_AT": "auto"}[k])
                      for k in _OPTION_NAMES}).replace(ACTIVATIONS=_D_ACTIVATIONS, TN_AT=_D_TN_AT)     # environment values are validated
