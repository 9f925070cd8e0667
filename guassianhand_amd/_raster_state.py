"""What the rasteriser remembers and decides between calls (no ctypes, no library). rasterizer.py is the module callers import."""
from __future__ import annotations

import os
import threading
import weakref
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import _abi


class GhOverflowError(RuntimeError):
    """The tile-instance capacity (max_instances) was too small for a sync-free call."""


class GhStaleGeometryError(GhOverflowError):
    """A static-geometry call (gh_forward_refresh) found an opacity above the bound its tile lists were built for: the lists
    may miss a tile. The call returned a NaN image (device-side guard, same mechanism as an instance overflow); every
    GeometryCache has been cleared, so re-running the step rebuilds the lists."""


class GhDepthBoundMiss(GhOverflowError):
    """A call with a speculative occlusion bound (DepthBoundCache) met a pixel that ran off the end of its truncated tile list: the
    Gaussians moved further than the margin allows. That pixel is NaN in the returned image; the bound has been dropped, re-run
    the step (it renders without a bound and produces a fresh one)."""


class DepthBoundCache:
    """Speculative per-tile occlusion bound for loops whose Gaussians move a LITTLE between steps — the one-shot fit's network-
    side trainables move them every step (infer_one_shot.py:340-343), so the static tile lists of GeometryCache cannot serve it.
    Every forward through the cache reports, per tile, the depth of the last list entry any pixel looked at (tiles whose pixels
    all reached the early stop; +inf elsewhere), times (1 + margin); the NEXT forward does not list instances behind it — on the
    hand scenes more than half of all instances lie behind a saturated surface and were emitted, sorted and gathered for nothing.
    The forward verifies the speculation per pixel (GhInputs.tile_depth_bound): where it holds the result is the unbounded
    call's bit for bit; where it fails the pixel is NaN, GhCounters.overflow bit 2 is set and the host re-runs without the bound
    (sync=True: transparently; sync-free: GhDepthBoundMiss from the backward / check_overflow). Not used inside captured graphs
    (the two buffers alternate between calls). margin: relative depth margin for the motion between two steps; slack: list
    entries kept behind the last one any pixel of the tile looked at. refresh_every: a forward that REPORTS a bound runs the
    kernel variant that walks on behind every pixel's stop until its transmittance has halved again (what tells a robustly
    saturated tile from one a rounding away from needing its whole list) — 26 % more forward time, measured; the bound is
    therefore refreshed every refresh_every-th call only and re-used in between (every call still verifies it; the margin has to
    cover the motion of that many steps). min_pixels: calls that render fewer pixels in all ignore the cache (the launch floors of a
    small call leave nothing for the bound to win: one 512x334 view 240 -> 257 us with it)."""

    def __init__(self, margin: float = 2e-3, slack: int = 8, refresh_every: int = 4, min_pixels: int = 4 * 512 * 334):
        self.margin, self.slack, self.refresh_every = float(margin), int(slack), max(1, int(refresh_every))
        self.min_pixels = int(min_pixels)        # calls smaller than this render without a bound (measured: one or two 512x334 views lose)
        self.bufs, self.key, self.cur, self.valid = None, None, 0, False
        self._cams, self._cams_version = None, None
        self.bounded_calls, self.misses, self.age = 0, 0, 0

    def clear(self) -> None:
        self.valid = False

    def _buffers(self, dev, NV: int, H: int, W: int, key=None):
        """(bound to apply or None, buffer to report into or None) for the next call; advances the cache's state.
        key = (P, per_view, packed camera tensor): a bound reported for OTHER cameras, another Gaussian count or the other
        Gaussian layout says nothing about this call (it would stay exact — the forward verifies — but miss on nearly every
        tile: a re-render under sync=True, a skipped step under sync=False), so the cache starts over when any of them changes.
        The cameras are identified by the tensor OBJECT and its version: pass the same packed tensor (camera.pack_cameras_from_w2c)
        every step for the bound to carry over."""
        P, per_view, cams = key if key is not None else (None, None, None)
        cam_ref = self._cams() if self._cams is not None else None
        same_cams = cams is None or (cam_ref is cams and self._cams_version == cams._version)
        full = (dev, NV, H, W, P, per_view)
        if self.key != full or not same_cams:
            T = NV * ((W + 15) // 16) * ((H + 15) // 16)
            if self.key is None or self.key[:4] != full[:4]:
                self.bufs = (torch.empty(T, 2, dtype=torch.float32, device=dev), torch.empty(T, 2, dtype=torch.float32, device=dev))   # (depth, block mask)
            self.key, self.cur, self.valid, self.age = full, 0, False, 0
            self._cams = None if cams is None else weakref.ref(cams)
            self._cams_version = None if cams is None else cams._version
        if self.valid and self.age + 1 < self.refresh_every:      # re-use the bound, plain kernels
            self.age += 1
            self.bounded_calls += 1
            return self.bufs[self.cur], None
        bound, seen = (self.bufs[self.cur] if self.valid else None), self.bufs[1 - self.cur]
        # the buffer this call writes is the next call's bound — also after a miss: a tile whose pixels did not all stop reports
        # +inf, so what the call leaves behind is a valid bound source either way
        self.cur, self.valid, self.age = 1 - self.cur, True, 0
        self.bounded_calls += 1 if bound is not None else 0
        return bound, seen


class GeometryCache:
    """Static geometry for calls that render the SAME Gaussians (means3D, scales, rotations, xyz_b) from the SAME cameras again
    and again while only opacities and colours move — the one-shot fit (infer_one_shot.py:489-524). The first call through a
    cache is a full forward with GH_FLAG_STATIC_LISTS; its context is kept here, and later calls whose geometry inputs are
    the very same tensor objects, unmodified (`is` + `_version`), go through gh_forward_refresh: no projection, no sorts.
    Anything else — another tensor, a bumped version, another image size — is a miss: a full call that replaces the entry.
    `clear()` forces the next call to rebuild (call it after changing a geometry tensor in place through `.data`, which
    `_version` cannot see). Opt-in: a caller passes its cache to rasterize_views / rendered_*_loss."""
    _all = weakref.WeakSet()

    def __init__(self):
        self.ctx, self.key, self.refs = None, None, None
        self.hits, self.builds = 0, 0
        GeometryCache._all.add(self)

    def clear(self) -> None:
        self.ctx, self.key, self.refs = None, None, None

    @staticmethod
    def clear_all() -> None:
        for c in list(GeometryCache._all):
            c.clear()

    def lookup(self, objs, vals):
        """The cached context if `objs` are the cached tensors, unmodified, and `vals` the cached scalars."""
        if self.ctx is None or self.key != vals or len(self.refs) != len(objs):
            return None
        for r, o in zip(self.refs, objs):
            if (r is None) != (o is None) or (r is not None and r() is not o):
                return None
        return self.ctx

    def store(self, objs, vals, ctx) -> None:
        self.refs = tuple(None if o is None else weakref.ref(o) for o in objs)
        self.key, self.ctx = vals, ctx


# ---------------------------------------------------------------------------------------------------
# What the rasteriser remembers between calls. Two kinds, kept apart (round 5):
#   * _DeviceState — per DEVICE, behind one re-entrant lock: learned instance capacities, the GH_FLAG_DEPTH24 verdicts, outstanding
#     counter read-backs, the workspace pool, the geometry record of the two-call protocol, graph-mode counters, the latest
#     workspace / gradient block. Two devices in one process share nothing; two threads on one device (autograd runs `backward` on
#     a thread of its own) take the lock around every read-modify-write of it.
#   * _Policy — process-wide SWITCHES a program sets once (graph mode, split-stream policy, geometry reuse, stage timing): plain
#     configuration, no per-call state.
# The module attributes earlier rounds' tests and tools read (`_capacity`, `_depth24`, `_geom_last`, `_graph_counters`, `_pending`,
# `_split_policy` ...) resolve to the CURRENT device's state through the module __getattr__ at the end of rasterizer.py.
class _DeviceState:
    def __init__(self, index: int):
        self.index = index
        self.lock = threading.RLock()
        # capacity policy for the data-dependent instance count D: call shape -> learned max_instances
        self.capacity: Dict[Tuple[int, int, int, int, bool], int] = {}
        # GH_FLAG_DEPTH24 (three depth-sort passes instead of four: two launches less per forward) per call shape. The flag is a
        # speculation the device can only answer with a NaN image, so it is used ONLY for a shape a read-back has shown it to hold
        # for (GhCounters.overflow bit 4, reported by every full forward, also one made WITHOUT the flag): absent = unknown = four
        # passes; True = observed to hold; False = observed to fail once (bit 3, or bit 4 missing): four passes from then on.
        self.depth24: Dict[Tuple[int, int, int, int, bool], bool] = {}
        self.pending = []        # _Pending records of sync-free calls not yet checked
        self.free_slots = []     # recycled (pinned 4-int buffer, event) pairs: a sync-free call allocates neither
        self.last_D = 0
        self.last_ws = None      # workspace of the most recent forward (its first 16 bytes are the GhCounters)
        self.graph_counters = {} # workspace address -> (device view of GhCounters, cap, key) of forwards issued in graph mode
        self.ws_pool: Dict[Tuple[int, int], list] = {}
        self.geom_last = None    # (identity objects, values, weakref to the context) of the latest full drop-in forward
        self.last_grad_block = None
        self.stage_events = []   # (stage name, start event, end event)


class _Policy:
    graph_mode = False
    split = False                # False | True | "auto"
    reuse_geometry = True
    stage_timing = False
    # raster_forward(l1_target=... / fit_loss=...) takes the render kernel's epilogue (GhOutputs.l1_* / fit_loss) where the library
    # offers it; GH_FUSED_LOSS=0 in the environment: measurement A/B (set_fused_loss)
    fused_loss = os.environ.get("GH_FUSED_LOSS", "1") != "0"


_policy = _Policy()
_states: Dict[int, _DeviceState] = {}
_states_lock = threading.Lock()


def _dev_index(dev=None) -> int:
    if dev is None:
        return torch.cuda.current_device() if torch.cuda.is_available() else 0
    if isinstance(dev, int):
        return dev
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _state(dev=None) -> _DeviceState:
    """The rasteriser's state for `dev` (a torch.device, an index, or None = the current device)."""
    i = _dev_index(dev)
    st = _states.get(i)
    if st is None:
        with _states_lock:
            st = _states.setdefault(i, _DeviceState(i))
    return st


class CounterWord(NamedTuple):
    """A forward's GhCounters as read back, decoded once (counter_word): what each path then does with it is its own policy."""
    d: int             # tile instances D
    bits: int          # GhCounters.overflow: error bits 0-3, information bit 4
    reserved0: int     # after a split call: the max_instances that would have given each half a large enough share (need())

    errors = property(lambda w: w.bits & _abi.GH_COUNTER_ERROR_MASK)
    overflow = property(lambda w: bool(w.bits & _abi.GH_COUNTER_OVERFLOW))            # D > max_instances (split: a half's share)
    stale = property(lambda w: bool(w.bits & _abi.GH_COUNTER_STALE_LISTS))            # a refresh met an opacity above its lists' bound
    bound_miss = property(lambda w: bool(w.bits & _abi.GH_COUNTER_BOUND_MISS))        # a pixel ran off a list the occlusion bound cut
    depth24_failed = property(lambda w: bool(w.bits & _abi.GH_COUNTER_DEPTH24_FAILED))
    depth24_ok = property(lambda w: bool(w.bits & _abi.GH_COUNTER_DEPTH24_OK))        # the depth keys' top byte did not vary

    def need(self, split: bool) -> int:       # the instance count that sizes the shape's next capacity
        return max(self.d, self.reserved0) if split else self.d


def counter_word(c4) -> CounterWord:           # c4: the host read-back of a GhCounters' int32 view
    return CounterWord(c4[0] & 0xFFFFFFFF, c4[1] & 0xFFFFFFFF, c4[2] & 0xFFFFFFFF)


def _learn_depth24(st: _DeviceState, key, flags_word: int, d: int = 1) -> None:
    """Update the GH_FLAG_DEPTH24 verdict of a call shape from a counter word that has been read back — the word of a FULL forward
    whose depth sort ran (callers pass nothing else: a refresh, a shared call or a call with nothing to project sorted nothing, and
    a word that says nothing must not decide anything). d: the call's instance count; with d = 0 no key took part in
    the (OR, AND) of the key bits, so "the top byte did not vary" is vacuous and "bit 4 absent" impossible: unknown stays unknown."""
    w = CounterWord(d, flags_word, 0)
    if w.depth24_failed:
        st.depth24[key] = False
    elif w.d == 0:
        return
    elif w.depth24_ok:
        st.depth24.setdefault(key, True)
    elif not w.overflow:                   # a complete call whose depths' top byte varies (truncated lists prove nothing)
        st.depth24[key] = False


def _grow_capacity(st: _DeviceState, key, need: int, floor: int = 0) -> None:
    """Raise the learned capacity of a call shape to hold `need` instances with room to spare (it never shrinks)."""
    st.capacity[key] = max(st.capacity.get(key, 0), int(need * 1.5) + 1024, floor)


_DEPTH24_MSG = ("the visible depths span more than the 24 key bits the three-pass depth sort covers; the call returned a NaN image; "
                "the four-pass sort is used for this call shape from now on, re-run the step")
_STALE_MSG = ("an opacity rose above the bound the static tile lists were built for; the call returned a NaN image; "
              "the geometry caches are cleared, re-run the step (it rebuilds the lists)")
_MISS_MSG = ("a pixel ran off the end of a tile list truncated by the speculative occlusion bound (the Gaussians moved further than "
             "the margin); that pixel is NaN; the bound has been dropped, re-run the step")
_PENDING_MAX = 64


class _Pending:
    """The asynchronous counter read-back of one sync-free forward. `resolve()` waits for it (normally long done), recycles
    the pinned buffer and remembers the verdict, so that both check_overflow() and the call's own backward can ask."""
    __slots__ = ("st", "ev", "host", "cap", "key", "done", "d", "over", "stale", "miss", "wide", "dbound", "told", "learn24")

    def __init__(self, st, ev, host, cap, key, dbound=None, learn24=True):
        self.st, self.ev, self.host, self.cap, self.key, self.dbound = st, ev, host, cap, key, dbound
        # the verdict, once resolved: D, any error bit, stale lists, a bound miss, GH_FLAG_DEPTH24 failed (CounterWord)
        self.done, self.d, self.over, self.stale, self.miss, self.wide = False, 0, False, False, False, False
        self.learn24 = learn24     # a full forward (the depth sort ran): its counter word says whether GH_FLAG_DEPTH24 holds
        self.told = False          # the caller has been given this record's error (a look at the counters by the geometry-reuse check is not that)

    def resolve(self) -> bool:
        """True when the call's counters hold an error bit (what the word says has been learned then)."""
        st = self.st
        with st.lock:
            if not self.done:
                self.ev.synchronize()
                w = counter_word(self.host.tolist())
                st.last_D = w.d
                if self.learn24:
                    _learn_depth24(st, self.key, w.bits, w.d)
                if w.bound_miss and self.dbound is not None:   # the speculation failed: the re-run of the step renders without a bound
                    self.dbound.clear()
                    self.dbound.misses += 1
                self.dbound = None
                if w.overflow or w.stale:                      # stale lists, or lists truncated by an instance overflow: never re-use them
                    GeometryCache.clear_all()
                if w.overflow:                                 # (a split call's reserved[0] sizes the next capacity)
                    _grow_capacity(st, self.key, w.need(self.key[-1]))
                st.free_slots.append((self.host, self.ev))
                self.host = self.ev = None
                self.d, self.over, self.stale, self.miss, self.wide = w.d, w.errors != 0, w.stale, w.bound_miss, w.depth24_failed
                self.done = True
        return self.over

    def kind(self):
        """(rank, exception class, message) of a bad record. Of several, check_overflow() raises the highest rank first: stale lists
        and a capacity overflow ask for a rebuild or a larger workspace, a depth-key verdict or a bound miss only for the step again."""
        capacity = (f"tile instances D={self.d} exceeded max_instances={self.cap}; the call returned a NaN image; "
                    "capacity raised, re-run the step")
        if self.stale:
            return 3, GhStaleGeometryError, _STALE_MSG
        if self.d > self.cap:
            return 2, GhOverflowError, capacity
        if self.miss:
            return 0, GhDepthBoundMiss, _MISS_MSG
        if self.wide:
            return 1, GhOverflowError, _DEPTH24_MSG
        return 0, GhOverflowError, capacity           # bit 0 alone with D <= max_instances: a split call's half outgrew its share

    def error(self) -> GhOverflowError:
        self.told = True
        _, exc, msg = self.kind()
        return exc(msg)


def _queue_readback(st: _DeviceState, counters, cap, key, dbound=None, learn24=True) -> _Pending:
    """Asynchronous copy of a call's GhCounters into a pinned buffer + an event: the record of a sync-free call."""
    host, ev = st.free_slots.pop() if st.free_slots else (torch.empty(4, dtype=torch.int32, pin_memory=True), torch.cuda.Event())
    host.copy_(counters, non_blocking=True)
    ev.record()
    pc = _Pending(st, ev, host, cap, key, dbound, learn24)
    st.pending.append(pc)
    return pc


def _record(st: _DeviceState, counters, cap, key, full: bool, dbound=None) -> Optional[_Pending]:
    """The record of a sync-free forward. Graph mode: none; its counters are registered for check_overflow (keyed by the workspace's
    address, so a workspace re-used by later captures is listed once). Else a read-back behind the bounded queue of unchecked ones.
    full: a full forward, whose depth sort ran (its word says whether GH_FLAG_DEPTH24 holds; a refresh's says nothing about it)."""
    if _policy.graph_mode:
        st.graph_counters[counters.data_ptr()] = (counters, cap, key, full)
        return None
    if len(st.pending) >= _PENDING_MAX:
        check_overflow(block=False, dev=st.index)
        if len(st.pending) >= _PENDING_MAX:
            check_overflow(block=True, dev=st.index)
    return _queue_readback(st, counters, cap, key, dbound, full)


# Four places read a counter word: _Pending.resolve / _Pending.kind and report_counter_word here, the sync branch of _forward_refresh
# and the retry loop of _forward_full in _raster_launch.py. They differ on purpose (tests/golden/counter_word_outcomes.json.gz):
#   * report_counter_word clears the geometry caches on ANY error bit; the sync-free record only on an overflow or stale lists;
#   * report_counter_word ranks a failed GH_FLAG_DEPTH24 above a capacity overflow; _Pending.kind ranks it below;
#   * _forward_full counts a bound miss only when no other error bit is set.
def report_counter_word(key, flags_word: int, d: int, cap: int, reserved0: int = 0, dev=None, where: str = "", learn24: bool = True) -> None:
    """Act on a GhCounters.overflow word read back from a workspace the caller holds itself (a captured graph's, see
    fit.CapturedFitStep.check): learn what it says (capacity, GH_FLAG_DEPTH24 verdict, stale caches) and raise the matching error.
    learn24: the word is a FULL forward's (its depth sort ran); a refresh over static lists passes False."""
    w = CounterWord(d, flags_word, reserved0)
    st = _state(dev)
    with st.lock:
        st.last_D = w.d
        if learn24 or w.depth24_failed:
            _learn_depth24(st, key, w.bits, w.d)
        if not w.errors:
            return
        GeometryCache.clear_all()                           # stale lists, or lists truncated by an overflow: never refreshed again
        if w.stale:                                         # a static-geometry replay met an opacity above its lists' bound
            raise GhStaleGeometryError(_STALE_MSG + where)
        if w.depth24_failed:                                # GH_FLAG_DEPTH24 did not hold for a captured call
            raise GhOverflowError(_DEPTH24_MSG + where)
        _grow_capacity(st, key, w.need(key[-1]))            # any other error bit: a larger capacity (reserved[0] sizes a split call's)
        raise GhOverflowError(f"tile instances D={w.d} exceeded max_instances={cap}" + (where or " inside a captured graph"))


def check_overflow(block: bool = True, keep_recent: int = 0, dev=None) -> None:
    """Verify every outstanding sync-free forward on `dev` (None = the current device) fitted its capacity (raises
    GhOverflowError). block=False only looks at read-backs that have arrived — except that all but the `keep_recent` latest
    calls are waited for regardless (they finished long ago), which bounds how late an overflow can surface."""
    st = _state(dev)
    with st.lock:
        for counters, cap, key, full in list(st.graph_counters.values()):   # graph mode: workspaces are static, read them directly
            w = counter_word(counters.tolist())
            report_counter_word(key, w.bits, w.d, cap, w.reserved0, dev=st.index,
                                where=" [inside a captured graph: capture again]" if (w.stale or w.depth24_failed) else "", learn24=full)
        keep, bad = [], []
        n_old = len(st.pending) - keep_recent if keep_recent > 0 else 0
        for i, pc in enumerate(st.pending):
            if pc.done:
                if pc.over and not pc.told:                    # resolved by somebody who did not report it (the geometry-reuse check)
                    bad.append(pc)
                continue
            if not block and i >= n_old and not pc.ev.query():
                keep.append(pc)
                continue
            if pc.resolve():
                bad.append(pc)
        if bad:
            # ONE error per call, the highest-ranked first (_Pending.kind); the records not reported now stay in the
            # list (resolved, untold) and surface at the next check instead of being dropped.
            worst = max(bad, key=lambda p: p.kind()[0])
            st.pending = [p for p in bad if p is not worst] + keep
            raise worst.error()
        st.pending = keep


def last_guard(dev=None):
    """Device view of the GhCounters of the most recent forward on `dev` (None = the current device): the `guard` argument of
    gh_l1_loss / gh_fit_loss / gh_adam_reg_step (device-side overflow guard). Holds that workspace alive until the next forward."""
    ws = _state(dev).last_ws
    return None if ws is None else ws[:16]


def last_num_rendered(dev=None) -> int:
    """Tile instances D of the most recent forward whose counters have been read back."""
    return _state(dev).last_D


def enable_stage_timing(on: bool) -> None:
    """Bracket every pipeline stage with HIP events on the launch stream (bench.py's roofline leg)."""
    _policy.stage_timing = bool(on)
    if on:
        for st in list(_states.values()):
            st.stage_events.clear()


def set_graph_mode(on: bool) -> None:
    """Graph mode: sync-free forwards issue no counter read-back at all (nothing but kernel launches and async
    memsets reaches the stream), so a whole step can be captured with torch.cuda.CUDAGraph / hipGraph.
    check_overflow() then reads the counters of the captured workspaces directly."""
    _policy.graph_mode = bool(on)
    if not on:
        for st in list(_states.values()):
            with st.lock:
                st.graph_counters.clear()


def graph_counters(dev=None):
    """[(device view of GhCounters, max_instances, call-shape key)] of the forwards issued in graph mode on `dev` so far — what a
    capture keeps to check its replays (fit.CapturedFitStep)."""
    st = _state(dev)
    with st.lock:
        return list(st.graph_counters.values())


_SPLIT_AUTO_MIN_PIXELS = 1 << 19   # "auto": where the split measured a gain (1024x1024 x 8 views: +4.9 %; 512x334: 8 views -1 %, 16 views +0.8 %)


def set_split_streams(mode) -> None:
    """Module policy for calls that do not say (split_streams=None): False = one stream, True = split whenever n_views >= 2,
    "auto" = split where it measured a gain: four or more views of more than half a megapixel each (GH_FLAG_SPLIT_STREAMS;
    results are bit-identical either way)."""
    if mode not in (False, True, "auto"):
        raise ValueError("set_split_streams: False, True or 'auto'")
    _policy.split = mode


def set_fused_loss(on: bool) -> None:
    """Module policy: let raster_forward(l1_target=...) — i.e. loss.rendered_l1_loss — take the image loss from the render kernel's
    own epilogue (GhOutputs.l1_*, the default) or always run gh_l1_loss on the stored image (measurement A/B; same gradients bit for
    bit, the loss up to the order of its float32 sums)."""
    _policy.fused_loss = bool(on)


def capacity_key(P: int, NV: int, H: int, W: int, split: bool = False):
    """Key of the learned instance capacity of a call shape (tests / tools)."""
    return (P, NV, H, W, bool(split))


def _initial_capacity(P: int, NV: int) -> int:
    return max(1 << 16, 8 * P * NV)


# Workspace pool: a forward takes its workspace from here and the context gives it back when it dies (after its backward,
# or when a no-grad caller drops it), so steady-state calls allocate nothing. Per device, keyed by (stream, bytes): a workspace
# only ever returns to the stream that used it last, and that stream orders its next use behind the previous one (callers
# that render on several streams at once — e.g. two half-batches overlapped in one captured graph — get one set per stream).
_WS_POOL_DEPTH = 4


def _ws_acquire(st: _DeviceState, dev: torch.device, nbytes: int, stream: int) -> torch.Tensor:
    with st.lock:
        free = st.ws_pool.get((stream, nbytes))
        if free:
            return free.pop()
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _ws_release(ws: Optional[torch.Tensor], stream: int) -> None:
    if ws is None:
        return
    st = _state(ws.device)
    with st.lock:
        free = st.ws_pool.setdefault((stream, ws.numel()), [])
        if len(free) < _WS_POOL_DEPTH:
            free.append(ws)


def clear_workspace_pool() -> None:
    for st in list(_states.values()):
        with st.lock:
            st.ws_pool.clear()


def last_grad_block(dev=None):
    """(block, n_reducible, spans, blend_end) of the most recent raster_backward: `block[:n_reducible]` is the contiguous fp32
    buffer [4 caller floats | every view-summed gradient] the kernels wrote in place, spans = [(name, shape, offset, numel)],
    block[:blend_end] = [4 caller floats | gradients of the blend parameters] (the prefix the one-shot fit reduces).
    The sharded fit all-reduces it directly (dist.allreduce_block): no torch.cat of the parts."""
    return _state(dev).last_grad_block


def set_geometry_reuse(on: bool) -> None:
    """The reference renders every view twice over identical geometry (RGB pass, then mask pass with colour 1 / bg 0,
    renderer_one_shot.py:338-346, :372-379). With reuse on (default) a drop-in call that receives the very same tensor
    objects (unmodified) for means3D / opacities / scales / rotations and the same camera as the previous call, with
    precomputed colours, shares the previous call's projection and tile lists (bit-identical results)."""
    _policy.reuse_geometry = bool(on)
    for st in list(_states.values()):
        with st.lock:
            st.geom_last = None
