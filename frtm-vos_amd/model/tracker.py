"""Sequence tracker (API of the reference's model/tracker.py:16-227).

Same control flow per frame -- backbone -> per-object coarse score -> refinement -> soft-max merge ->
per-object memory/filter update -- with the device work re-laid out for one MI355X:
 * one native trunk call per frame; during ``initialize`` the trunk stops after the tap the
   discriminator reads (the reference also runs resnet.layer4 there for nothing);
 * all objects go through the refiner in one batched pass; the object-independent half of it is
   computed once per frame;
 * merge (clamp / background / soft-max / arg-max, tracker.py:214-221) is one HIP kernel, in place;
 * the trunk does not depend on tracking state, so ``run_sequence`` feeds it ``feature_batch`` pre-loaded frames at a time
   (default 16, as ``trunk_lanes`` = 2 concurrent sub-batches of 8): at batch 1 the 30x54 / 15x27 stages cannot fill 256 CUs
   (47 TFLOP/s, many split-K convs), at batch 4 they do (80 TFLOP/s, no split-K), and two sub-batches on two streams cover
   each other's kernel tails (the last, partly filled round of workgroups of every launch): 95 TFLOP/s.  Per-frame results
   are unchanged up to fp32 summation order; ``track(image)`` without pre-computed features still works frame by frame;
 * between two filter re-solves (8 frames) nothing but the memory inserts carries state from frame to frame, so ``run_sequence``
   scores and refines those frames as ONE window of frames x objects samples (``track_window``); merge, pixel counts, memory
   inserts and the re-solve follow frame by frame in order;
 * the "fewer than 10 pixels" early-out of Discriminator.update (discriminator.py:214) is evaluated for all objects by
   one kernel; on frames without a filter re-solve it guards the memory insert on the device (no host sync at all), on
   re-solve frames (every 8th) ONE small device->host copy serves all objects.
"""
from contextlib import contextmanager
from time import time

import numpy as np
import os
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .. import _hip as H
from ..lib.utils import AverageMeter
from .discriminator import Discriminator, apply_grouped, leave_resident_forms


_STREAMS = {}


def _process_stream(device, role):
    """Side streams are shared by all trackers of a process (one per device and role: 'main', 'first', 'init0'..).  A tracker that took
    fresh streams from torch's 32-stream pool for itself left hipGraphs behind that had been captured on ever different streams, and the
    HIP runtime crashed inside hipGraphLaunch once the pool had wrapped around a few times in a process that creates and destroys many
    trackers / refiners (the test suite; reproducer tools/graph_stress.py).  Trackers of one process do not run concurrently (one host
    thread drives them), so they can share."""
    key = (torch.device(device).index, role)
    if os.environ.get('FRTM_PRIVATE_STREAMS'):
        return torch.cuda.Stream(device=device)
    if key not in _STREAMS:
        _STREAMS[key] = torch.cuda.Stream(device=device)
    return _STREAMS[key]


STREAM_PROBE = {}       # role -> {probed, independent}: what the placement found (bench.py reports it)


def _streams_are_independent(a, b, busy_us=400):
    """Does work enqueued on stream ``b`` start while stream ``a`` is busy?  The HIP runtime maps the streams of a process onto a few hardware
    queues (GPU_MAX_HW_QUEUES, 4 by default); two streams that landed on the SAME queue execute in order, whatever their events say.
    Measured in round 4 (tools/timeline_now.sh, per-queue strip chart): the tracker's main stream shared a queue with the stream of the
    first tracking pass, so the first-frame augmentation -- a host-bound chain of small kernels that the early pass is there to cover --
    waited for the whole pass and the GPU then idled through it (2 ms of a 46 ms sequence).  The probe: two dependent 0.4 ms spin
    kernels on ``a``, a 1 us kernel + event on ``b``; independent streams complete the event within the launch latency."""
    from time import perf_counter
    L = H.lib()
    torch.cuda.synchronize()
    for _ in range(2):
        if L.frtm_spin(int(busy_us), a.cuda_stream) != 0:
            return True
    L.frtm_spin(1, b.cuda_stream)
    ev = torch.cuda.Event()
    ev.record(b)
    t0 = perf_counter()
    while not ev.query() and perf_counter() - t0 < 4e-6 * busy_us:
        pass
    dt = perf_counter() - t0
    torch.cuda.synchronize()
    return dt < 0.6e-6 * busy_us


def _independent_stream(device, role, others, tries=6):
    """The process-wide stream of ``role`` (see _process_stream), chosen at its first use among pool streams such that it shares its
    hardware queue with none of ``others`` (streams that carry work at the same time).  Falls back to the first candidate when no
    independent one turns up in ``tries``; FRTM_NO_STREAM_PROBE=1 takes the first candidate unprobed (the behaviour up to round 3)."""
    key = (torch.device(device).index, role)
    if os.environ.get('FRTM_PRIVATE_STREAMS') or key in _STREAMS:
        return _process_stream(device, role)
    if int(os.environ.get('FRTM_NO_STREAM_PROBE', '0') or 0):
        STREAM_PROBE[role] = dict(probed=False, independent=False)
        return _process_stream(device, role)              # (`others` is not even evaluated: stream creation order as up to round 3)
    others = [o for o in (others() if callable(others) else others) if o is not None]
    probe = bool(others) and not torch.cuda.is_current_stream_capturing()
    first, found = None, False
    with torch.cuda.device(torch.device(device)):
        for _ in range(tries if probe else 1):
            c = torch.cuda.Stream(device=device)
            if any(c == s_ for s_ in _STREAMS.values()):     # (the pool has wrapped around: this one already serves another role)
                continue
            first = first if first is not None else c
            if not probe or all(_streams_are_independent(o, c) for o in others):
                _STREAMS[key], found = c, probe
                break
        else:
            _STREAMS[key] = first if first is not None else torch.cuda.Stream(device=device)
    STREAM_PROBE[role] = dict(probed=probe, independent=found)
    return _STREAMS[key]


@contextmanager
def persistent_taps(ext, lanes, use_graph, also=()):
    """The trunk ``ext`` writes its taps into persistent buffers for the duration, ``lanes`` sub-batches at a time, replayed as hipGraphs
    or not; ``also``: further (object, attribute, value) settings for the duration.  Everything but the lane count is put back afterwards:
    a caller that holds two results of ext() (no_grad_forward's chunks, user code) must not find them aliased.  Yields whether the taps
    are persistent; a caller-supplied extractor without ``reuse_outputs`` is left alone."""
    if not hasattr(ext, 'reuse_outputs'):
        yield False
        return
    settings = [(ext, 'reuse_outputs', True), (ext, 'use_graph', use_graph)] + list(also)
    saved = [(o, a, getattr(o, a)) for o, a, _ in settings]
    for o, a, v in settings:
        setattr(o, a, v)
    if ext.lanes != lanes:
        ext.lanes = lanes
    try:
        yield True
    finally:
        for o, a, v in saved:
            setattr(o, a, v)


def update_targets(active, cfts, masks, counts, update_filters, windowed):
    """Memory inserts and filter re-solves after W tracked frames, frame by frame in order.  ``masks`` (W,n_obj+1,H,W) merged,
    ``cfts[k]`` (W,c,h,w) projected features of active[k] -- None: the scoring has advanced the target models itself (apply_grouped) --,
    ``counts`` (W,n_obj+1) device int32 pixels per plane, or None: counted here.  ``windowed``: one batched update per object
    (Discriminator.update_window) when every insert and the re-solve at the end are decided on the device."""
    W, K = masks.shape[:2]

    def advance(f):
        for k, t in enumerate(active if cfts is not None else ()):
            t.discriminator.advance(cfts[k] if W == 1 else cfts[k][f:f + 1])

    def on_device():
        return all(t.discriminator.guards_on_device() for t in active)
    if not (active and update_filters):
        for f in range(W):
            advance(f)
        return
    if counts is None:
        counts = ops.count_above(masks.reshape(W * K, *masks.shape[-2:])).view(W, K)     # device int32, no sync
    if windowed and on_device() and masks.is_contiguous() and all(t.discriminator.can_update_window(W) for t in active):
        for k, t in enumerate(active):
            t.discriminator.update_window(cfts[k], masks, t.index, counts)
        return
    flat = counts.view(-1)
    for f in range(W):
        advance(f)
        solve = any(t.discriminator.frame_num % t.discriminator.train_skipping == 0 for t in active)
        host = counts[f].tolist() if solve and not on_device() else None                 # (no D2H at all when the early-out runs on the device)
        for t in active:
            i = t.index                                                                  # (one view each: (1,1,H,W) plane, (1,) count)
            t.discriminator.update(masks[f:f + 1, i:i + 1], num_positive=None if host is None else host[i], count_dev=flat[f * K + i:f * K + i + 1])


def fused_step(refiner, frame_targets, feats, size, update_filters, windowed=False, scores=None, masks=None, counts=None,
               lut=None, single=False, grouped=None, table=None):
    """The tracking step of F frames of n objects each when every mask plane comes from the refiner (Tracker.fused_tail): scores into
    one frame-major batch, refiner, then sigmoid + merge + pixel counts + label decoding as ONE kernel (ops.track_merge), then
    update_targets.  ``frame_targets[f]``: the n TargetObjects of frame f; consecutive frames that share a list are scored as one
    window.  track(): F = 1; track_window(): W frames, one list; a StreamPool group: one list per stream.  ``scores`` / ``masks`` /
    ``counts``: the caller's buffers (else allocated); ``lut``: labels are decoded through it; ``grouped`` = (table cache, cft workspace):
    one grouped launch scores all pairs (apply_grouped; every frame has its own list).  -> (masks (F,n+1,H,W), labels (F,1,H,W) or None).
    Frames whose lists differ in length (a StreamPool group of streams with different object counts) take the same step on the indexed
    launches: one ops.RaggedTable (``table``: the caller's, else built here) serves the grouped scoring, the refiner and
    ops.track_merge_ragged; ``scores`` is then (N,1,h,w) with N the sum of the counts and ``masks`` (N + F,H,W) / ``counts`` (N + F) are
    packed, frame f's n_f + 1 planes at table.planes(f).  No labels there: -> (masks packed, None)."""
    F_, n = len(frame_targets), len(frame_targets[0])
    ft = feats[frame_targets[0][0].disc_layer]
    dev = ft.device
    if F_ > 1 and any(len(ts) != n for ts in frame_targets):
        if lut is not None:
            raise ValueError('fused_step: no label decoding for frames with different object counts')
        return _fused_step_ragged(refiner, frame_targets, feats, size, update_filters, scores, masks, counts, grouped, table), None
    if scores is None:
        scores = torch.empty(F_ * n, 1, *ft.shape[-2:], device=dev)
    cuts = [f for f in range(F_) if f == 0 or frame_targets[f] is not frame_targets[f - 1]] + [F_]
    runs = list(zip(cuts[:-1], cuts[1:]))
    part = (lambda t, a, b: t) if len(runs) == 1 else (lambda t, a, b: t[a:b])           # (no view of the whole: track() is bound by the host)
    if grouped is not None:
        apply_grouped([t.discriminator for ts in frame_targets for t in ts], ft, n, grouped[0], cft=grouped[1], scores=scores)
        cfts = [None] * F_
    else:
        cfts = [[t.discriminator.apply_window(part(feats[t.disc_layer], f0, f1), interleave=(part(scores, f0 * n, f1 * n), k, n))[0]
                 for k, t in enumerate(frame_targets[f0])] for f0, f1 in runs]
    logits = refiner(scores, feats, size)                                                # (F*n,1,H,W), frame-major
    if masks is None:
        masks = torch.empty(F_, n + 1, *size, device=dev)
    labels = torch.empty(F_, 1, *size, dtype=torch.uint8, device=dev) if lut is not None else None
    if counts is None and update_filters:
        counts = torch.empty(F_, n + 1, dtype=torch.int32, device=dev)
    ops.track_merge(logits, F_, n, masks, labels, lut, single, counts)
    masks = masks.view(F_, n + 1, *size)
    for (f0, f1), cft in zip(runs, cfts):
        update_targets(frame_targets[f0], cft, part(masks, f0, f1), None if counts is None else part(counts, f0, f1), update_filters, windowed)
    return masks, labels


def _fused_step_ragged(refiner, frame_targets, feats, size, update_filters, scores, masks, counts, grouped, table):
    """fused_step for frames whose lists differ in length (see there): one refiner pass and one merge for all of them.  -> masks packed."""
    ft = feats[frame_targets[0][0].disc_layer]
    dev = ft.device
    cnts = tuple(len(ts) for ts in frame_targets)
    if table is None:
        table = ops.RaggedTable(cnts, dev)
    elif table.counts != cnts:
        raise ValueError('fused_step: the table holds %r objects per frame, the frames %r' % (table.counts, cnts))
    F_, N = table.F, table.n
    if scores is None:
        scores = torch.empty(N, 1, *ft.shape[-2:], device=dev)
    if grouped is not None:
        apply_grouped([t.discriminator for ts in frame_targets for t in ts], ft, table, grouped[0], cft=grouped[1], scores=scores)
        cfts = [None] * F_
    else:                                                                                # each frame's targets into its slice of the batch
        cfts = [[t.discriminator.apply_window(feats[t.disc_layer][f:f + 1], interleave=(scores[table.starts[f]:table.starts[f + 1]], k, len(ts)))[0]
                 for k, t in enumerate(ts)] for f, ts in enumerate(frame_targets)]
    logits = refiner(scores, feats, size, frame_of=table)                                # (N,1,H,W), frame-major
    if masks is None:
        masks = torch.empty(N + F_, *size, device=dev)
    if counts is None and update_filters:
        counts = torch.empty(N + F_, dtype=torch.int32, device=dev)
    ops.track_merge_ragged(logits, table, masks, counts)
    for f, ts in enumerate(frame_targets):
        a, b = table.planes(f)
        update_targets(ts, cfts[f], masks[a:b].unsqueeze(0), None if counts is None else counts[a:b].unsqueeze(0), update_filters, False)
    return masks


class FrameTaps(dict):
    """Backbone taps of one frame ({layer: (1,C,H,W)}) that remember the trunk batch they are a slice of, so that consecutive
    frames can be handed on as one window without copying."""

    def __init__(self, batch, k):
        super().__init__({L: t[k:k + 1] for L, t in batch.items()})
        self.batch, self.k = batch, k
        self.last = k + 1 == next(iter(batch.values())).shape[0]      # last frame of its trunk batch


class TargetObject:

    def __init__(self, obj_id, disc_params, discriminator=None, **kwargs):
        self.object_id = obj_id
        # `discriminator`: a recycled instance (Tracker.release_targets); it re-draws its weights like a new one would
        self.discriminator = discriminator.recycle() if discriminator is not None else Discriminator(**disc_params)
        self.disc_layer = disc_params.layer
        self.start_frame = None
        self.start_mask = None
        self.index = -1
        for key, val in kwargs.items():
            setattr(self, key, val)

    def initialize(self, ft, mask):
        self.discriminator.init(ft[self.disc_layer], mask)

    def classify(self, ft, interleave=None):
        return self.discriminator.apply(ft, interleave=interleave)


def _tensor_frames_only(who, images):
    """The sequence paths read decoded files: their frames are tensors."""
    if any(isinstance(im, ops.DecoderFrame) for im in images):
        raise TypeError('%s takes tensor frames only; an ops.DecoderFrame goes through Tracker.initialize / track or a StreamPool' % who)


class Tracker(nn.Module):

    def __init__(self, augmenter, feature_extractor, disc_params, refiner, device, feature_batch=16, trunk_lanes=2, refiner_graphs=False,
                 working_size=None):
        super().__init__()
        # working_size (h, w): frames of any other size are resized to it on the device (mode 'area', csrc/frame_resize.hip; the first-frame
        # label map nearest), every step and all state (current_masks, memories, target models) live at that size, and track() /
        # run_sequence answer at the frame's native size (ops.masks_to_native, csrc/native_size.hip).  None (default): every path, launch
        # and bit as without the option; so is a frame that already has the working size.
        if working_size is not None:
            working_size = tuple(int(v) for v in working_size)
            if len(working_size) != 2 or not all(1 <= v <= ops.MAX_NATIVE_DIM for v in working_size):
                raise ValueError('working_size must be (h, w) with 1 <= h, w <= %d, got %r' % (ops.MAX_NATIVE_DIM, working_size))
        self.working_size = working_size
        self._resize_plans = {}          # (kind, frames, native size) -> (ops.ResizePlan, output buffer or None); ('decoder', size, pitch, uv offset, format) -> (ops.FramePlan, buffer)
        self._native_tables = {}         # (frames, planes, native size, soft) -> ops.NativeTable
        self._native_bufs = {}           # (planes, native size) -> (labels, soft): what track() answers with, valid until its next call
        self._native_lut = None          # (object ids, device uint8 LUT) of track()'s native label map
        self.native_labels = None        # track() under working_size: the (1, H, W) uint8 label map of the frame at its native size
        self.feature_batch = feature_batch
        self.trunk_lanes = trunk_lanes   # concurrent sub-batches of a trunk pass (frtm_backbone_set_lanes)
        self.graph_trunk = False         # trunk passes replayed as hipGraphs: nothing to gain since the host no longer waits for the GPU
                                         # while tracking (64 frames: 498 vs 499 frames/s), and every new batch shape costs a capture
                                         # (30 DAVIS-like sequences: 350 frames/s with lazily captured trunk graphs, 378 without)
        self.overlap_first_pass = False  # first trunk pass of a sequence on a side stream, next to initialize()'s fits (measured: no gain
                                         # with 2 objects -- the fits just run slower next to the trunk kernels --, +3 % with 5)
        self._after_init_trunk = None
        self._first_stream = None
        self._main_stream = None
        self.own_stream = True           # run_sequence moves off the framework's default (null) stream
        self.window_tracking = True      # track the frames between two filter re-solves as one batch (track_window)
        self.init_lanes = 4              # objects starting on the same frame are fitted on up to this many concurrent streams
        # ... in the chain form when exactly this many start together (else: resident fits, one after the other); 0 = never
        self.concurrent_chain_fits = int(os.environ.get('FRTM_CONCURRENT_CHAIN_FITS', '3'))
        self.share_first_sample = True   # the un-augmented frame (sample 0 of every object's stack) passes the trunk once per frame
        self.early_first_pass = True     # first tracking pass enqueued before initialize(): it runs under the host-bound augmentation
        # ... and initialize()'s own pass could run NEXT TO it on the trunk's second lane set (frtm_backbone_forward_at).  OFF: measured in
        # round 4 (20-frame sequence, tools/timeline_init.sh): with the runtime's default 4 hardware queues the tracker's stream shares a queue
        # with a trunk lane and runs behind it anyway; with GPU_MAX_HW_QUEUES=8 the two passes do overlap ([0, 29.3] and [3.4, 18.9] ms) but
        # finish no earlier than one after the other (30.2 ms): four lanes share the GPU at 110 TFLOP/s, and more hardware queues slow
        # everything else down (397 instead of 415 frames/s at 8, 350 at 16).
        self.concurrent_init_pass = bool(os.environ.get('FRTM_CONCURRENT_INIT_PASS'))
        self._early_pass_event = None
        self._init_pool = []
        self._disc_pool = []
        # Refiner windows replayed as hipGraphs: OPT-IN since round 6 (constructor argument refiner_graphs=True).  What a replay gained over
        # launching the ~80 kernels of a window one by one was the overlap of the deep pyramid levels with the 120x214 level, not the launch
        # count (the host enqueues ahead of the GPU) -- and the eager path now forks them onto the shared side stream itself
        # (SegNetwork.parallel_eager; profiles/r06_refiner_window_ab.txt: 8 frames x 2 objects 3.03 ms serial, 2.87 eager-parallel, 2.89 replayed).
        # Twice in round 5 a test process died inside hipGraphLaunch replaying such a graph; tools/graph_repro.hip (pure HIP: capture across
        # pooled / destroyed streams and events, replay of graphs whose streams are gone, destruction in flight; 2000-3000 iterations per mode)
        # does not reproduce it (profiles/r06_graph_repro.txt), so the cause is NOT named and the default path does not replay graphs.
        # Same kernels either way: results are bit-identical (tests/test_round6_gpu.py).
        self.graph_refiner = bool(refiner_graphs)
        # No cyclic garbage collection while a sequence is being enqueued (_run_sequence).  A process-global side effect, so OPT-IN: the
        # drivers (bench.py, evaluate.py) switch it on; an embedding application keeps its collector unless it sets this or FRTM_HOLD_GC=1.
        self.hold_gc = bool(os.environ.get('FRTM_HOLD_GC')) and not os.environ.get('FRTM_NO_HOLD_GC')
        self.prefetch_sequences = True   # run_dataset: the next sequence is decoded / copied to the device while this one is tracked
        self.prefetch_stream = False     # True: next trunk batch on a side stream, overlapped with tracking (+3.5 % fps measured)
        self.pipeline_passes = False     # two tap sets, passes one ahead on a side stream, a short pass before and a pass beside
                                         # initialize()'s fits (supersedes early_first_pass / overlap_first_pass / prefetch_stream)
        self.first_batch = None          # frames of the pipelined first pass (default: feature_batch // 2)
        self.fold_tail = max(0, int(feature_batch) // 4 - 1)   # a last trunk batch of at most this many frames is folded into the one before it
        self.balance_batches = False     # True: trunk batches of similar size instead of full ones and a short tail (batch_sizes).  Measured
                                         # at 20 frames: the 8 + 11 split saves 2 ms of trunk time but the long first pass no longer covers
                                         # initialize()'s host-bound phases: 58 instead of 54 ms per sequence
        self.augmenter = augmenter
        self.augment = augmenter.augment_first_frame
        self.disc_params = disc_params
        self.feature_extractor = feature_extractor
        self.refiner = refiner
        for m in self.refiner.parameters():
            m.requires_grad_(False)
        self.refiner.eval()
        self.device = H.normalize_device(device)   # 'cuda' -> 'cuda:<current>': side streams, prefetcher and frame views compare devices by index
        self.first_frames = []
        self.current_frame = 0
        self.current_masks = None
        self.num_objects = 0
        self.targets = dict()
        # Optional callable(obj_id) -> (project.weight, filter.weight): weights a new target model STARTS from INSTEAD of the default.
        # The default is the reference's: drawn from the process-global CPU generator when the object appears, which initialize() seeds
        # with 0 after every object like the reference does (tracker.py:174-180) -- so every target model but a process's first starts
        # from one fixed draw (model/discriminator.py: _start_weights, fixture G15).  Parity tests that want DIFFERENT weights per
        # object (fixtures G12 / G14) inject them here on both sides.
        self.start_weights = None
        self.frame_views = not os.environ.get('FRTM_NO_FRAME_VIEW')     # consecutive pre-loaded frames reach the trunk as a view (no gather)
        self.fuse_merge = not os.environ.get('FRTM_NO_FUSE_MERGE')    # sigmoid + merge + pixel counts + label decoding of a window as ONE kernel (ops.track_merge)
        self._lut = None                 # run_sequence: device uint8 table mask plane -> object id (label decoding inside the merge kernel)
        self._single = False
        self._window_labels = None
        self._raw_log = None             # list: (frame, masks before the merge) of every tracked frame is appended (ytvos merge, parity tests)
        self._unchecked_fits = []        # targets whose first-frame fit has not been asked for a timed-out resident launch yet
        self._in_run_sequence = False    # run_sequence asks after the sequence (_check_first_frame_fits), track() before the frame
        self._rerun = False              # the sequence is being tracked again after a resident launch timed out
        self.object_ids = None
        self.last_enqueue_seconds = 0.0

    def release_targets(self):
        """Ends a sequence: the target models go back to a pool and serve the next sequence's objects, so that the steady
        state allocates nothing on the device (hipMalloc / hipFree stall the queue for milliseconds at arbitrary moments)."""
        for t in self.targets.values():
            if t.discriminator is not None and len(self._disc_pool) < 64:
                self._disc_pool.append(t.discriminator)
                t.discriminator = None
        self.targets = dict()

    def _first_pass_stream(self):
        if self._first_stream is None:
            # next to it run: the stream that called (initialize()'s augmentation and fits) and the trunk's own lane streams
            self._first_stream = _independent_stream(self.device, 'first', lambda: [torch.cuda.current_stream(self.device)] + self._trunk_lane_streams())
        return self._first_stream

    def busy_streams(self):
        """The streams a sequence's GPU work runs on (main, first tracking pass, the trunk's lanes): what a copy stream should keep off."""
        if not torch.cuda.is_available() or torch.device(self.device).type != 'cuda':
            return []
        if self._main_stream is None and self.own_stream:
            self._main_stream = _independent_stream(self.device, 'main', self._trunk_lane_streams)
        main = self._main_stream if self._main_stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(main):
            first = self._first_pass_stream()
        return [main, first] + self._trunk_lane_streams()

    def _trunk_lane_streams(self):
        ext = self.feature_extractor
        fn = getattr(ext, 'lane_streams', None)       # (a caller-supplied extractor need not have lanes)
        if fn is None:
            return []
        if hasattr(ext, 'reuse_outputs'):             # the lane count run_sequence is about to set (the lane streams exist from then on)
            ext.lanes = max(1, min(int(self.trunk_lanes), max(1, int(self.feature_batch))))
        return list(fn())

    def _init_streams(self, n):
        while len(self._init_pool) < n:
            # (default priority: high-priority streams measured 2.4x SLOWER for these chains on MI355X / ROCm 7.2: 41 vs 17 ms)
            # each on a hardware queue of its own as far as the runtime's queues go: fits that share a queue run one after the other
            prev = list(self._init_pool)
            self._init_pool.append(_independent_stream(self.device, 'init%d' % len(self._init_pool), lambda: prev))
        return self._init_pool[:n]

    def clear(self):
        self.first_frames = []
        self.current_frame = 0
        self.current_masks = None
        self.num_objects = 0
        self.native_labels = None

    # ---- working size ------------------------------------------------------------------
    def _off_size(self, image):
        """Does this frame take the way in and back: is a working size set, and has the frame another size?"""
        return self.working_size is not None and tuple(image.shape[-2:]) != self.working_size

    def _step_size(self, image):
        """The size the tracking step of this frame runs at."""
        return self.working_size if self.working_size is not None else image.shape[-2:]

    def _resize_in(self, images, keep=False):
        """(B,3,H,W) uint8 frames of one native size -> (B,3,h,w) at the working size in ONE launch (mode 'area').  ``keep``: into a buffer
        kept per (B, native size), valid until the next such call (the per-frame callers); else a fresh tensor."""
        if images.dtype != torch.uint8:
            raise TypeError('working_size: frames are uint8 (the resize kernel reads bytes), got %s' % images.dtype)
        B, native = images.shape[0], tuple(images.shape[-2:])
        key = ('frames', B, native, bool(keep))
        plan = self._resize_plans.get(key)
        if plan is None:
            n = 3 * native[0] * native[1]
            desc = torch.tensor([[i * n, native[0], native[1], ops.RESIZE_MODES['area']] for i in range(B)], dtype=torch.int64)
            buf = torch.empty((B, 3) + self.working_size, dtype=torch.uint8, device=self.device) if keep else None
            plan = self._resize_plans[key] = (ops.ResizePlan(desc, self.device), buf)
        return plan[0].frames(images.to(self.device).contiguous().view(-1), 3, self.working_size, out=plan[1])

    def _resize_first(self, image, labels):
        """The first frame (or a later one on which objects start) and its label map at the working size: the frame 'area', the ids nearest."""
        native = tuple(image.shape[-2:])
        if not torch.is_tensor(labels) or labels.dtype != torch.uint8:
            raise TypeError('working_size: the label map is a uint8 tensor (the resize kernel reads bytes), got %s' % getattr(labels, 'dtype', type(labels).__name__))
        im = self._resize_in(image.reshape(1, 3, *native), keep=True).view(tuple(image.shape[:-2]) + self.working_size)
        return im, self._resize_labels(labels, native)

    def _resize_labels(self, labels, native):
        """A uint8 label map at ``native`` size -> the working size, ids nearest."""
        if not torch.is_tensor(labels) or labels.dtype != torch.uint8:
            raise TypeError('working_size: the label map is a uint8 tensor (the resize kernel reads bytes), got %s' % getattr(labels, 'dtype', type(labels).__name__))
        key = ('labels', 1, native, False)
        plan = self._resize_plans.get(key)
        if plan is None:
            plan = self._resize_plans[key] = (ops.ResizePlan(torch.tensor([[0, native[0], native[1], 0]], dtype=torch.int64), self.device), None)
        lb = plan[0].label_map(labels.to(self.device).contiguous().view(-1), self.working_size)
        return lb.view(tuple(labels.shape[:-2]) + self.working_size)

    def _decode(self, frame):
        """An ops.DecoderFrame -> its (3, h, w) uint8 RGB planes at the step size in ONE launch (ops.FramePlan: colour conversion fused
        into the resize, mode 'area'; at the frame's own size the conversion alone).  Plan and buffer are kept per (size, pitch, uv offset,
        format): a steady loop allocates nothing, and the planes are valid until the next frame of that layout is decoded."""
        size = tuple(int(v) for v in self._step_size(frame))
        key = ('decoder',) + frame.plan_key()
        plan = self._resize_plans.get(key)
        if plan is None:
            desc = torch.tensor([frame.row(0, 'area')], dtype=torch.int64)
            plan = self._resize_plans[key] = (ops.FramePlan(desc, self.device), torch.empty((1, 3) + size, dtype=torch.uint8, device=self.device))
        return plan[0].frames(frame.data, size, out=plan[1])[0]

    def _object_lut(self):
        """Device uint8 table mask plane -> object id of the objects known so far (plane 0: the background, id 0)."""
        ids = tuple(int(t.object_id) for t in sorted(self.targets.values(), key=lambda t: t.index))
        if self._native_lut is None or self._native_lut[0] != ids:
            if any(not 0 <= i < 256 for i in ids):
                raise ValueError('working_size: object ids are 0 .. 255 (uint8 label maps), got %r' % (ids,))
            self._native_lut = (ids, H.upload(torch.tensor((0,) + ids, dtype=torch.uint8), self.device))
        return self._native_lut[1]

    def _to_native(self, masks, native, lut, soft, keep=False):
        """Merged masks (F,K,h,w) at the working size -> (labels (F,1,H,W) uint8, soft (F,K,H,W) or None) at ``native`` in ONE launch
        (ops.masks_to_native).  ``keep``: into buffers kept per shape, valid until the next such call; else fresh tensors."""
        masks = masks.contiguous()
        F_, K = masks.shape[:2]
        native = (int(native[0]), int(native[1]))
        key = (F_, K, native, bool(soft))
        table = self._native_tables.get(key)
        if table is None:
            table = self._native_tables[key] = ops.NativeTable.packed(self.working_size, [(K,) + native] * F_, self.device, soft=soft, shared_lut=True)
        bufs = self._native_bufs.get(key) if keep else None
        if bufs is None:
            bufs = (torch.empty(table.label_bytes, dtype=torch.uint8, device=self.device),
                    torch.empty(table.soft_elems, device=self.device) if soft else None)
            if keep:
                self._native_bufs[key] = bufs
        ops.masks_to_native(masks, table, bufs[0], lut, soft=bufs[1])
        return bufs[0].view(F_, 1, *native), (bufs[1].view(F_, K, *native) if soft else None)

    # ------------------------------------------------------------------------------------
    def run_dataset(self, dataset, out_path, speedrun=False, restart=None, writer=None):
        """Reference tracker.py:68-101.  ``writer(path, label_image)`` stores a palette PNG; default: the
        package's own imwrite_indexed (lib/image.py of the reference is I/O, out of the hot path)."""
        if writer is None:
            from ..lib.image import imwrite_indexed as writer
        out_path.mkdir(exist_ok=True, parents=True)
        dset_fps = AverageMeter()
        print('Evaluating', dataset.name)
        from ..lib.datasets import SequencePrefetcher

        def todo():
            restarted = False
            for sequence in dataset:
                if restart is not None and not restarted:
                    if sequence.name != restart:
                        continue
                    restarted = True
                yield sequence
        # sequence.preload(device) of the reference (:91) -- for the NEXT sequence, on a copy stream, while this one is tracked
        for sequence in SequencePrefetcher(todo(), self.device, enabled=self.prefetch_sequences, avoid=self.busy_streams):
            self.clear()
            outputs, seq_fps = self.run_sequence(sequence, speedrun)
            dset_fps.update(seq_fps)
            dst = out_path / sequence.name
            dst.mkdir(exist_ok=True)
            for lb, f in zip(outputs, sequence.frame_names):
                writer(dst / (f + '.png'), lb)
        print('Average frame rate: %.2f fps' % dset_fps.avg)
        return dset_fps.avg

    def prewarm(self, size, object_counts=(1, 2, 3), seed=0):
        """Optional: pay the one-off costs (kernel code objects, trunk arenas, the hipGraphs of every trunk batch / tracking
        window shape) for frames of ``size`` and the given numbers of objects BEFORE any timed sequence, on synthetic frames.
        A sequence then only replays.  Sequence lengths are chosen so that every window length 1..8 and a full trunk batch occur."""
        from ..lib.synthetic import SyntheticSequence
        fb = max(1, int(self.feature_batch))
        ext, ref = self.feature_extractor, self.refiner
        saved = (getattr(ext, 'capture_after', None), getattr(ref, 'capture_after', None))
        if saved[0] is not None:
            ext.capture_after = 0                            # capture at first sight (normally: from the second use on)
        if saved[1] is not None:
            ref.capture_after = 0
        try:
            for n in object_counts:
                for residual in range(1, 9):
                    seq = SyntheticSequence('prewarm', 1 + fb + residual, tuple(size), n, seed=seed + n)
                    seq.preload(self.device)
                    self.run_sequence(seq)
        finally:
            if saved[0] is not None:
                ext.capture_after = saved[0]
            if saved[1] is not None:
                ref.capture_after = saved[1]
        self.release_targets()
        torch.cuda.synchronize()

    def run_sequence(self, sequence, speedrun=False, ytvos_merge=False):
        """Reference tracker.py:103-163: frames / wall-clock of the loop below, initialize() included.  Called on the framework's
        DEFAULT stream, the sequence runs on a stream of this tracker instead: the default stream is the legacy null stream, which
        synchronises implicitly with every blocking stream of the process -- measured: the first host-side read of initialize()
        waited 18 ms for a trunk-graph replay in flight on the side stream.  The caller's stream waits for the results."""
        cur = torch.cuda.current_stream(self.device) if torch.cuda.is_available() and torch.device(self.device).type == 'cuda' else None
        if cur is None or cur != torch.cuda.default_stream(self.device) or not self.own_stream:
            return self._run_sequence(sequence, speedrun, ytvos_merge)
        if self._main_stream is None:
            self._main_stream = _independent_stream(self.device, 'main', self._trunk_lane_streams)
        self._place_refiner_side_stream()
        self._main_stream.wait_stream(cur)
        with torch.cuda.stream(self._main_stream):
            out = self._run_sequence(sequence, speedrun, ytvos_merge)
        cur.wait_stream(self._main_stream)
        for o in out[0]:                                     # the label images were allocated on this tracker's stream and are
            if torch.is_tensor(o) and o.is_cuda:             # now the caller's: tell the allocator who reads them
                o.record_stream(cur)
        return out

    def _place_refiner_side_stream(self):
        """The refiner's shared side stream (deep pyramid levels next to the 120x214 level, model/seg_network.py: _shared_side_stream) on a
        hardware queue other than the tracker's main stream's: streams of one queue run in order, the fork would buy nothing."""
        from . import seg_network as SN
        idx = torch.device(self.device).index
        if idx not in SN._SIDE and hasattr(self.refiner, 'parallel_eager'):
            SN._SIDE[idx] = _independent_stream(self.device, 'refiner_side', lambda: [self._main_stream])

    def _run_sequence(self, sequence, speedrun=False, ytvos_merge=False):
        """_run_sequence_loop with the interpreter's cyclic garbage collector held off (``hold_gc``): the host enqueues a sequence's
        few thousand launches AHEAD of the GPU (a 20-frame sequence: 17 ms of host work for 46 ms of GPU work), and a generation-2
        collection of a PyTorch process (1.7e5 tracked objects here) stops it for 40-50 ms -- whenever one fell into a short sequence
        the GPU ran dry and that sequence came out at 270-330 instead of 420 frames/s (the sporadic "slow runs" of rounds 2 and 3,
        every GPU stage timer normal).  Reference counting still frees everything that is not a cycle; cycles wait for the end of the
        sequence.  Only this SCOPED disable / enable lives in the library, and only when ``hold_gc`` is set (off by default); moving the
        long-lived objects into the permanent generation (gc.freeze) is the DRIVER's decision, once per process
        (``frtm_vos_amd.lib.utils.freeze_long_lived_objects``, called by bench.py and evaluate.py)."""
        import gc
        if not self.hold_gc:
            return self._run_sequence_loop(sequence, speedrun, ytvos_merge)
        was = gc.isenabled()
        gc.disable()
        try:
            return self._run_sequence_loop(sequence, speedrun, ytvos_merge)
        finally:
            if was:
                gc.enable()

    def _run_sequence_loop(self, sequence, speedrun=False, ytvos_merge=False):
        """The loop of run_sequence on the current stream.

        ``ytvos_merge``: label decoding of the reference's YouTube-VOS validation fork instead (ytvos_validation/tracker.py:84-116):
        the per-object masks BEFORE the per-frame merge are kept for the whole sequence, the ground truth is re-inserted on every
        object's first frame, and ONE merge over the sequence (background = min(1 - p), soft-max of p / (1 - p), arg-max) gives the
        labels.  Tracking itself (scores, refinement, per-frame merge for the memory updates) is unchanged."""
        if ytvos_merge and self.working_size is not None:
            raise ValueError("run_sequence: ytvos_merge with working_size is not supported (the fork's sequence-level merge at native size)")
        self.eval()
        self._raw_log = [] if ytvos_merge else None
        self.object_ids = sequence.obj_ids
        self.current_frame = 0
        self.release_targets()
        self._in_run_sequence, self._unchecked_fits = True, []
        try:
            return self._run_sequence_frames(sequence, speedrun, ytvos_merge)
        finally:
            self._in_run_sequence, self._unchecked_fits = False, []

    def _run_sequence_frames(self, sequence, speedrun, ytvos_merge):
        N = 0
        object_ids = H.upload(torch.tensor([0] + list(sequence.obj_ids), dtype=torch.uint8), self.device)
        self._lut, self._single = object_ids, len(sequence.obj_ids) == 1
        if speedrun:
            image, labels, obj_ids = sequence[0]
            _tensor_frames_only('run_sequence', [image])
            self.initialize(image.to(self.device), labels.to(self.device), sequence.obj_ids)
            self.track(image.to(self.device))
            torch.cuda.synchronize()
            self.release_targets()
        outputs = []
        window = []                                          # frames waiting to be tracked together: (image, taps)

        def decode(masks):
            """(W,n_obj+1,H,W) merged masks -> (W,1,H,W) uint8 label images (tracker.py:143-150), the whole window at once."""
            if len(sequence.obj_ids) == 1:
                return object_ids[(masks[:, 1:2] > 0.5).long()]
            return object_ids[ops.merge_masks_(masks.clone()).argmax(dim=1, keepdim=True)]   # :146-150 (merge of merged masks)

        def flush():
            if window:
                masks_w = self.track_window([im for im, _ in window], [ft for _, ft in window])
                # (the merge kernel has decoded the labels on the way when all planes came from the refiner; else: the ATen form)
                if self._off_size(window[0][0]):             # native-size label maps of the whole window in one launch, no soft planes
                    labels_w = self._to_native(masks_w, window[0][0].shape[-2:], object_ids, soft=False)[0]
                else:
                    labels_w = self._window_labels if self._window_labels is not None else decode(masks_w)
                for f in range(labels_w.shape[0]):
                    outputs.append(labels_w[f])
                    self.current_frame += 1
                del window[:]

        t0 = time()
        for i, (image, labels, new_objects, feats) in enumerate(self.frames_with_features(sequence)):
            image = image.to(self.device)
            if len(new_objects) > 0:
                flush()                                      # everything before this frame, with the old set of objects
                had_objects = len(self.targets) > 0
                labels = labels.to(self.device)
                self.initialize(image, labels, new_objects)
                if had_objects:
                    window.append((image, feats))
                    flush()                                  # this frame on its own: the set of active objects changes after it
                else:
                    outputs.append(labels)
                    self.current_frame += 1
            elif len(self.targets) > 0:
                if window and not self._extends(window[-1][1], feats):
                    flush()
                window.append((image, feats))
                if self._window_complete(len(window), image) or getattr(feats, 'last', True):
                    flush()                                  # (also at the end of a trunk batch: its taps are about to be overwritten)
            else:
                if isinstance(labels, list) and len(labels) == 0:
                    labels = image.new_zeros(1, *image.shape[-2:])
                outputs.append(labels)
                self.current_frame += 1
            N += 1
        flush()
        if ytvos_merge:
            outputs = self._ytvos_labels(sequence, outputs, object_ids)
        self.last_enqueue_seconds = time() - t0              # host done; the GPU may still be working (no host wait while tracking)
        torch.cuda.synchronize()
        # Resident launches that timed out (another process holds CUs; a few bytes read per object, after the synchronise above).  A missed
        # filter re-solve has been made up on a later frame at best, a missed Gauss-Newton iteration of a first-frame fit not at all: frames
        # were tracked with a model the reference would not have had.  Every check is EVALUATED (each books its counters), then the sequence
        # is tracked again -- once: the resident forms are off for the rest of the process after the first time-out.
        discs = [t.discriminator for t in self.targets.values() if t.discriminator is not None]
        late = [d.recover_from_abort() for d in discs]
        if any(late):
            torch.cuda.synchronize()
        missing = [d.init_aborted() for d in discs]
        if (any(missing) or any(late) or any(d.num_persistent_aborts > 0 for d in discs)) and not self._rerun:
            leave_resident_forms()
            self._rerun = True
            try:
                self.release_targets()
                self.clear()
                return self._run_sequence_loop(sequence, speedrun, ytvos_merge)
            finally:
                self._rerun = False
        T = time() - t0
        self._raw_log = None
        self._lut = None
        return outputs, N / T

    def _ytvos_labels(self, sequence, outputs, object_ids):
        """Sequence-level decoding (ytvos_validation/tracker.py:103-116).  self._raw_log holds, per tracked frame, the masks before
        the merge: plane t.index = sigmoid(refiner) of an active object (already multiplied by (1 - start mask) of objects starting
        on that frame, :148-151), or the start mask itself on an object's first frame (= the re-inserted ground truth, :107-110)."""
        n = len(sequence.obj_ids)
        T_, (Hh, Ww) = len(outputs), outputs[0].shape[-2:]
        planes = torch.zeros(T_, n + 1, Hh, Ww, device=self.device)
        index = {t.object_id: t.index for t in self.targets.values()}
        for t_idx, raw in self._raw_log:
            planes[t_idx, :raw.shape[0]] = raw                          # planes of objects that do not exist yet stay 0
        for oid, t in self.targets.items():                             # objects whose first frame was not tracked (frame 0)
            planes[t.start_frame, index[oid]] = t.start_mask.reshape(Hh, Ww).float()
        ops.merge_masks_(planes)                                        # one launch over all frames: planes[:, 0] = background
        labels = object_ids[planes.argmax(dim=1, keepdim=True)]
        return [labels[t] for t in range(T_)]

    @staticmethod
    def _extends(prev, nxt):
        """Are the taps `nxt` the slice right after `prev` in the same trunk batch (one window = one contiguous slice)?"""
        return (isinstance(prev, FrameTaps) and isinstance(nxt, FrameTaps) and nxt.batch is prev.batch and nxt.k == prev.k + 1)

    def _window_complete(self, length, image):
        """A window ends with the frame on which some object re-solves its filter (the frames before it all see the same filter,
        reference discriminator.py:221-227), or when it holds as many samples as the refiner's 32-bit buffer offsets allow."""
        active = self.active_targets()
        if not self.window_tracking or not active:
            return True
        if any(t.discriminator.frames_until_solve() <= length for t in active if t.discriminator.update_filters):
            return True
        Hh, Ww = self._step_size(image)
        per_sample = 4 * 64 * (Hh // 2 + 1) * (Ww // 2 + 1)      # largest refiner activation of one sample (bytes)
        return (length + 1) * len(active) * per_sample > 0x7fffffff or length >= 64

    def frames_with_features(self, sequence):
        """Yields (image, labels, new_objects, taps).  The trunk runs on up to ``feature_batch`` consecutive frames at once.
        Single stream (default): a pass is enqueued when its first frame is asked for; the taps live in ONE persistent set of
        buffers, which the next pass overwrites -- run_sequence therefore tracks every frame of a batch before it asks for the
        first frame of the next one (tracking windows end with their trunk batch).  With ``prefetch_stream`` the pass of the NEXT
        batch runs on a side stream, into a second tap set, while the current batch is tracked (off by default: no gain, the
        trunk kernels saturate the GPU either way).  Frame 0 of a sequence is never tracked (only initialised), so its taps
        are not computed."""
        frames = list(sequence)
        _tensor_frames_only('frames_with_features', [f[0] for f in frames])
        fb = max(1, int(self.feature_batch))
        ext = self.feature_extractor
        also = [(self.refiner, 'use_graphs', self.graph_refiner)] if hasattr(self.refiner, 'use_graphs') else []
        with persistent_taps(ext, max(1, min(int(self.trunk_lanes), fb)), self.graph_trunk, also) as persistent:
            yield from self._frames_with_features(frames, fb, ext, persistent)

    def _frame_batch(self, ims):
        """(B,3,H,W) uint8 batch of consecutive frames for the trunk.  Sequences pre-load their frames as slices of ONE device tensor
        (lib/datasets.py, lib/synthetic.py): consecutive frames are then a view of it -- no gather kernel; anything else is stacked."""
        base = ims[0]._base if self.frame_views else None
        if (base is not None and base.is_cuda and base.device == torch.device(self.device) and ims[0].is_contiguous() and base.dim() == ims[0].dim() + 1
                and all(im._base is base for im in ims)):
            n, o0 = ims[0].numel(), ims[0].storage_offset()
            if n > 0 and (o0 - base.storage_offset()) % n == 0 and all(im.storage_offset() == o0 + i * n for i, im in enumerate(ims)):
                k0 = (o0 - base.storage_offset()) // n
                view = base[k0:k0 + len(ims)]
                if view.is_contiguous():
                    return view
        return torch.stack([im.to(self.device) for im in ims])

    def batch_sizes(self, n, fb):
        """Trunk batches for n tracked frames, fb frames each (the last one up to fb + fold_tail).  With ``balance_batches``: at most
        fb frames each, as few passes as possible, and those of similar size -- a
        3-frame tail pass after a 16-frame one runs at 76 TFLOP/s, two passes of 8 and 11 frames at 100-110 -- with the cuts on
        filter re-solve frames (multiples of ``train_skipping``) where that fits, so that no tracking window is split by a cut."""
        if n <= 0:
            return []
        k = -(-n // fb)
        if k == 1 or not self.balance_batches:
            sizes = [min(fb, n - i) for i in range(0, n, fb)]
            # a tail of a few frames does not fill the GPU (3 frames: 77 TFLOP/s against 113 for 16): it joins the pass before it
            if len(sizes) > 1 and sizes[-1] <= int(self.fold_tail):
                sizes[-2:] = [sizes[-2] + sizes[-1]]
            return sizes
        q = max(1, int(getattr(self.disc_params, 'train_skipping', 8)))
        cuts, prev = [], 0
        for j in range(1, k):
            ideal = n * j / k
            c = int(round(ideal / q)) * q
            lo, hi = max(prev + 1, n - (k - j) * fb), min(prev + fb, n - (k - j))     # what keeps every batch within 1..fb
            if not lo <= c <= hi:
                c = min(max(int(round(ideal)), lo), hi)
            cuts.append(c)
            prev = c
        edges = [0] + cuts + [n]
        return [b - a for a, b in zip(edges[:-1], edges[1:])]

    def _frames_with_features(self, frames, fb, ext, persistent):
        pipelined = bool(persistent and self.pipeline_passes and torch.cuda.is_available())
        side = None
        if pipelined:
            side = self._first_pass_stream()
        elif persistent and self.prefetch_stream and torch.cuda.is_available():
            side = _independent_stream(self.device, 'prefetch', lambda: [torch.cuda.current_stream(self.device)] + self._trunk_lane_streams())
        # trunk batches [first, last) over the tracked frames 1..; pipelined: a short first batch (it has to be through the trunk
        # before initialize()'s own pass can start)
        n_tracked = len(frames) - 1
        if pipelined:
            fb0 = max(1, min(fb, int(self.first_batch) if self.first_batch else max(1, fb // 2)))
            sizes, left = [], n_tracked
            while left > 0:
                sizes.append(min(left, fb0 if not sizes else fb))
                left -= sizes[-1]
        else:
            sizes = self.batch_sizes(n_tracked, fb)
        bounds, i0 = [], 1
        for size in sizes:
            bounds.append((i0, i0 + size))
            i0 += size
        pending = {}                                        # batch start -> (taps, ready event, frame indices)

        def launch(bi, on=None):
            if bi >= len(bounds) or bounds[bi][0] in pending:
                return
            i0 = bounds[bi][0]
            idx = list(range(*bounds[bi]))
            batch = self._frame_batch([frames[j][0] for j in idx])
            if self._off_size(batch):
                batch = self._resize_in(batch)               # the whole trunk batch to the working size in one launch
            st = on if on is not None else side
            if st is not None:
                st.wait_stream(torch.cuda.current_stream())         # the input batch (and the previous use of this tap set)
                with torch.cuda.stream(st):
                    ext.output_set = (bi & 1) if side is not None else 0
                    taps = ext(batch)
                    ev = torch.cuda.Event()
                    ev.record(st)
                batch.record_stream(st)
                if on is not None:
                    self._early_pass_event = ev          # initialize() runs its own pass NEXT TO this one (second lane set) and waits here before the fits
            else:
                if persistent:
                    ext.output_set = 0              # single tap set: the refiner's graphs stay keyed to 4 slice addresses
                taps, ev = ext(batch), None
            pending[i0] = (taps, ev, idx)

        # Single stream: a pass is enqueued when its first frame is asked for -- by then run_sequence has flushed every window of the
        # previous batch (windows end with the last frame of a trunk batch), so the one persistent tap set can be overwritten.
        # Side stream: one pass AHEAD, into the other tap set.
        starts_with_init = len(frames) > 1 and len(frames[0][2]) > 0
        if pipelined:
            # Two tap sets, every pass on the side stream, one pass ahead of the frames being tracked.  Around initialize():
            #   pass 0 (short) is enqueued BEFORE it and runs under its host-bound augmentation (a dozen tiny kernels and two
            #     device->host reads per object, which only synchronise the main stream);
            #   initialize()'s own pass (the augmented stacks) follows it (passes are serialised by the extractor);
            #   pass 1 is enqueued by the hook right after that and runs NEXT TO the target-model fits -- dependent chains of small
            #     kernels that leave most of the GPU idle on their own.
            launch(0)
            if starts_with_init:
                self._after_init_trunk = lambda: launch(1)
        elif (side is None and persistent and self.early_first_pass and not self.overlap_first_pass and torch.cuda.is_available()
                and starts_with_init):
            # The first tracking pass does not depend on initialize(): enqueue it right away on a side stream.  It then runs
            # while the host is busy with the first-frame augmentation, initialize()'s own trunk call follows it.  One pass only:
            # later passes reuse the single tap set.
            launch(0, on=self._first_pass_stream())
        elif side is not None:
            if len(frames) > 0 and len(frames[0][2]) > 0:
                # frame 0 initialises objects: its own trunk call (the augmented stacks) goes first, the pass for frames 1.. follows
                # on the side stream, next to the target-model fits (initialize() fires the hook right after its trunk call)
                self._after_init_trunk = lambda: launch(0)
            else:
                launch(0)
        elif persistent and self.overlap_first_pass and torch.cuda.is_available():
            # initialize() calls this hook right after it has enqueued its own trunk call: the pass then runs on a side stream
            # next to the target-model fits instead of after them.  One pass only: later passes overwrite the tap set in use.
            first = self._first_pass_stream()
            self._after_init_trunk = lambda: launch(0, on=first)
        cache, bi = {}, 0
        for i, (image, labels, new_objects) in enumerate(frames):
            feats = None
            if i > 0:
                if i not in cache:
                    launch(bi)                              # no-op when the pass is already in flight (side stream / init hook)
                    taps, ev, idx = pending.pop(i)
                    if ev is not None:
                        torch.cuda.current_stream().wait_event(ev)
                    cache = {j: FrameTaps(taps, k) for k, j in enumerate(idx)}
                    bi += 1
                    if side is not None:
                        launch(bi)                          # next batch runs on the side stream while this one is being tracked
                feats = cache.pop(i)
            yield image, labels, new_objects, feats
            self._after_init_trunk = None                   # only armed while frame 0 is being initialised

    # ------------------------------------------------------------------------------------
    @torch.no_grad()
    @H.roctx('initialize')
    def initialize(self, image, labels, new_objects):
        """Reference tracker.py:165-191.  Under ``working_size`` a frame of another size and its label map are resized first: the
        augmentation and the fits run at the working size, and so does the mask stack returned.  ``image`` may be an ops.DecoderFrame
        (the label map stays a uint8 tensor at the picture's size): it is converted -- and resized, in the same launch -- first."""
        if isinstance(image, ops.DecoderFrame):
            if self._off_size(image):
                labels = self._resize_labels(labels, tuple(image.shape[-2:]))
            image = self._decode(image)
        elif self._off_size(image):
            image, labels = self._resize_first(image, labels)
        Hh, Ww = image.shape[-2:]
        self.current_masks = H.fill(torch.empty((len(self.targets) + len(new_objects) + 1, Hh, Ww), device=self.device), 0.0)
        lab8 = labels.reshape(Hh, Ww)
        # the one-kernel mask path reads uint8 label maps; any other integer type (object ids beyond 255 exist in such maps, and a narrowing
        # cast would wrap them onto small ids) takes the reference's literal comparison below
        lab8 = lab8.contiguous() if lab8.dtype == torch.uint8 else None
        fresh, started = [], []
        for obj_id in new_objects:
            # mask = (labels == obj_id) as uint8 and as the object's plane of current_masks: one kernel (reference :170-172,188)
            if lab8 is not None and 0 <= int(obj_id) < 256:
                mask = torch.empty(1, Hh, Ww, dtype=torch.uint8, device=self.device)
                H.call('frtm_label_mask', lab8.data_ptr(), int(obj_id), Hh * Ww, mask.data_ptr(),
                       self.current_masks[len(self.targets) + 1].data_ptr())
            else:
                mask = (labels.reshape(1, Hh, Ww) == obj_id).to(torch.uint8)
                self.current_masks[len(self.targets) + 1].copy_(mask[0])
            target = TargetObject(obj_id=obj_id, index=len(self.targets) + 1, disc_params=self.disc_params,
                                  discriminator=self._disc_pool.pop() if self._disc_pool else None,
                                  start_frame=self.current_frame, start_mask=mask)
            self.targets[obj_id] = target
            if self.start_weights is not None:
                w1, w2 = self.start_weights(obj_id)
                d = target.discriminator
                d.project.weight.data.copy_(w1.to(d.project.weight.dtype))
                d.filter.weight.data.copy_(w2.to(d.filter.weight.dtype))
                d._invalidate()
            torch.random.manual_seed(0)        # the reference's "HACK for debugging" (:179-180) is kept (the next object's weights
            started.append((target, mask))     # are drawn from this state; the augmentation below draws from numpy only)
        # Telea's hole fill is a host step of a few ms per object (model/augmenter.py): the fills of objects that start TOGETHER run on host
        # threads at once instead of one after the other (only when self.augment still is the augmenter's own method, or says it wraps it)
        if len(started) > 1 and hasattr(self.augmenter, 'prefetch_fills') and \
                (self.augment == self.augmenter.augment_first_frame or getattr(self.augment, 'wraps_augmenter', False)):
            self.augmenter.prefetch_fills(image, [m for _, m in started])
        try:
            for target, mask in started:
                np.random.seed(0)              # augmentation draws are identical for every object (reference :180)
                im, msk = self.augment(image, mask)
                fresh.append((target, im, msk))
        finally:
            if hasattr(self.augmenter, 'drop_fills'):
                self.augmenter.drop_fills()    # (fills of objects whose augmentation raised are not kept for a later frame)
        if fresh:
            # one trunk call for the augmented stacks of ALL objects that start on this frame (the reference runs one per
            # object, :186); same per-image results, larger launches and one lane per object
            layers = sorted({t.disc_layer for t, _, _ in fresh})
            # Sample 0 of every object's augmented stack is the frame itself (augment_first_frame's contract, reference
            # augmenter.py:546-547): it goes through the trunk ONCE for all objects that start here, not once per object.
            share = self.share_first_sample and len(fresh) > 1
            # (opt-in, concurrent_init_pass: with the first tracking pass in flight on a side stream this pass takes the trunk's SECOND lane
            # set and runs next to it instead of behind it; measured: no gain, see __init__)
            early = self._early_pass_event if self.concurrent_init_pass else None
            kw = dict(lane_set=1) if early is not None else {}      # (a caller-supplied extractor need not know about lane sets)
            def gather(parts):                  # (torch.cat without its framework kernel: device-to-device copies into one batch)
                out = torch.empty((sum(p.shape[0] for p in parts),) + tuple(parts[0].shape[1:]), dtype=parts[0].dtype, device=parts[0].device)
                o = 0
                for p in parts:
                    out[o:o + p.shape[0]].copy_(p)
                    o += p.shape[0]
                return out
            if share:
                ft_all = self.feature_extractor(gather([fresh[0][1][:1]] + [im[1:] for _, im, _ in fresh]), layers, **kw)
            else:
                ft = self.feature_extractor(gather([im for _, im, _ in fresh]), layers, **kw)
            if early is not None:
                # the fits wait for the tracking pass: a resident fit wants every CU (two of them next to trunk kernels time out)
                torch.cuda.current_stream().wait_event(early)
            self._early_pass_event = None
            if self._after_init_trunk is not None:
                hook, self._after_init_trunk = self._after_init_trunk, None
                hook()
            # the objects' fits are independent chains of small kernels: enqueue them round-robin on side streams so that
            # they overlap on the GPU (reference :186-187 runs them one after the other)
            cur = torch.cuda.current_stream()
            lanes = self._init_streams(min(len(fresh), self.init_lanes)) if len(fresh) > 1 and self.init_lanes > 1 else []
            # THREE objects starting together: their fits in the CHAIN form on three concurrent streams beat the resident fits one after the other
            # (one fit's kernels run in the other fits' latency gaps): 342-346 -> 348-354 frames/s over 20 frames, alternating runs on one box.
            # Two objects are faster resident (430-432 against 425-428), and so are one (9.9 against 10.7 ms per initialize()) and four or more
            # (37.5 against 40.3 ms for five: four chain fits at once oversubscribe the GPU).  The stand-alone initialize() sweep ranks two
            # objects the other way round (16.1 against 16.6 ms): in a sequence the fits share the GPU with the first tracking pass.
            concurrent_chain = bool(lanes) and self.concurrent_chain_fits > 0 and len(fresh) == self.concurrent_chain_fits
            for target, _, _ in fresh:
                target.discriminator.resident_joint = not concurrent_chain
            if lanes:
                # resident fits (one launch per Gauss-Newton iteration, all CUs each) go one after the other on this stream
                fshape = (ft_all if share else ft)[fresh[0][0].disc_layer].shape
                if fresh[0][0].discriminator.resident_init(fresh[0][1].shape[0], fshape[-2], fshape[-1]):
                    lanes = []
            for st in lanes:
                st.wait_stream(cur)
            b0 = 1 if share else 0
            for i, (target, im, msk) in enumerate(fresh):
                k = im.shape[0] - 1 if share else im.shape[0]
                # fits that share the GPU on concurrent streams keep their first filter fit in the chain form: resident launches of several
                # objects next to each other starve one another's grids (measured with the resident joint form switched off and five
                # objects: two of the first fits timed out and the process fell back to the chain form for good)
                target.discriminator.persistent_first_fit = type(target.discriminator).persistent_first_fit and not lanes
                def fit(target=target, msk=msk, b0=b0, k=k):
                    # (the gather of the shared sample runs on the stream of the fit that reads it)
                    feats = ({L: gather((ft_all[L][:1], ft_all[L][b0:b0 + k])) for L in layers} if share
                             else {L: ft[L][b0:b0 + k] for L in layers})
                    target.initialize(feats, msk)
                if lanes:
                    with torch.cuda.stream(lanes[i % len(lanes)]):
                        fit()
                else:
                    fit()
                b0 += k
            for st in lanes:
                cur.wait_stream(st)
            self._unchecked_fits = self._unchecked_fits + [t for t, _, _ in fresh]
        return self.current_masks

    def _check_first_frame_fits(self):
        """Callers that own the frame loop (initialize() / track(), the reference's contract): before the first frame is tracked with a new
        target model, ask whether a resident launch of its first-frame fit timed out (Discriminator.init_aborted: waits for the fit, a few
        bytes read) and restart the fit in the chain form right away -- no frame is ever scored with a half-fitted model.  run_sequence
        does not wait here (its host runs whole sequences ahead of the GPU): it asks after the sequence and tracks it again."""
        fits, self._unchecked_fits = self._unchecked_fits, []
        for t in fits:
            d = t.discriminator
            if d is not None and self.targets.get(t.object_id) is t and d.init_aborted():
                d.refit_in_chain_form()

    def active_targets(self):
        """The objects tracked on the current frame: those that started before it."""
        return [t for t in self.targets.values() if t.start_frame < self.current_frame]

    def fused_tail(self, active):
        """Does every plane of the mask stack come from the refiner (no object starts on this frame, no raw masks are being logged)?  Then
        the tail of the step is ONE kernel (fused_step); otherwise the step-by-step form (_track_stepwise)."""
        n = len(active)
        return bool(self.fuse_merge and active and n == len(self.targets) and n < 16 and self._raw_log is None
                    and all(t.index == k + 1 for k, t in enumerate(active)))

    def _track_stepwise(self, active, feats, size, W, windowed):
        """The tracking step of W frames in the reference's steps (tracker.py:198-221), on W copies of ``current_masks``."""
        masks = self.current_masks.unsqueeze(0).repeat(W, 1, 1, 1) if W > 1 else self.current_masks.unsqueeze(0)
        cfts = []
        if active:
            n = len(active)
            per_obj = [t.discriminator.apply_window(feats[t.disc_layer]) for t in active]          # (W,c,h,w), (W,1,h,w)
            cfts = [c for c, _ in per_obj]
            scores = torch.stack([s for _, s in per_obj], dim=1).reshape(W * n, 1, *per_obj[0][1].shape[-2:])   # frame-major
            y = torch.sigmoid(self.refiner(scores, feats, size)).view(W, n, *size)
            for k, t in enumerate(active):
                masks[:, t.index] = y[:, k]
        for t1 in active:                                                                        # :208-212 (only when W == 1)
            for t2 in self.targets.values():
                if t2 is not t1 and t2.start_frame == self.current_frame:
                    masks[0, t1.index] *= (1 - t2.start_mask.squeeze(0)).float()
        if self._raw_log is not None:
            for f in range(W):
                self._raw_log.append((self.current_frame + f, masks[f].clone()))
        ops.merge_masks_(masks)                                                                  # :214-221, all frames of the window
        update_targets(active, cfts, masks, None, self.disc_params.update_filters, windowed)
        return masks

    @torch.no_grad()
    @H.roctx('track_window')
    def track_window(self, images, taps):
        """track() for W consecutive frames at once (one contiguous slice of a trunk batch, same active objects, no filter
        re-solve before the last frame): one projection / score / refiner pass over W x n samples instead of W passes over n.
        Per frame the arithmetic is that of track(); the memory inserts and the re-solve run frame by frame afterwards, in order
        (as one batched update per object when that is decided on the device).
        Returns the per-frame ``current_masks`` stacked: (W, n_obj+1, H, W)."""
        _tensor_frames_only('track_window', images)
        W = len(images)
        im_size = self._step_size(images[0])
        first = taps[0]
        feats = {L: first.batch[L][first.k:first.k + W] for L in first.batch} if isinstance(first, FrameTaps) else first
        active = self.active_targets()
        self._window_labels = None
        if self.fused_tail(active):
            # (the score maps are written straight into the refiner's (frame, object) batch; the merge kernel decodes the labels on the way)
            masks, self._window_labels = fused_step(self.refiner, [active] * W, feats, im_size, self.disc_params.update_filters,
                                                    windowed=True, lut=None if self._off_size(images[0]) else self._lut, single=self._single)
        else:
            masks = self._track_stepwise(active, feats, im_size, W, windowed=True)
        self.current_masks = masks[W - 1]
        return masks

    @torch.no_grad()
    def track(self, image, features=None):
        """Reference tracker.py:193-227.  ``features``: optional pre-computed taps of this frame (frames_with_features).  Under
        ``working_size`` a frame of another size is resized, the step runs at the working size (``current_masks`` stays there) and the
        answer is the (n_obj + 1, H, W) stack at the frame's native size, valid until the next call; ``native_labels`` is its label map.
        ``image`` may be an ops.DecoderFrame: one launch converts it and takes it to the step size, the rest is what a tensor frame gets."""
        decoder = isinstance(image, ops.DecoderFrame)
        if self._off_size(image):
            native = tuple(image.shape[-2:])
            if decoder:
                image = self._decode(image) if features is None else None
            elif features is None:                                 # (with the taps given, the image only names the native size)
                image = self._resize_in(image.reshape(1, 3, *native), keep=True).view(tuple(image.shape[:-2]) + self.working_size)
            self._track(image, features, self.working_size)
            labels, soft = self._to_native(self.current_masks.unsqueeze(0), native, self._object_lut(), soft=True, keep=True)
            self.native_labels = labels[0]
            return soft[0]
        self.native_labels = None                                  # (this frame's answer is current_masks itself)
        size = image.shape[-2:]
        if decoder:
            image = self._decode(image) if features is None else None
        return self._track(image, features, size)

    def render_answer(self, image, labels):
        """(answer, lut or None) of ops.render_frames for ``image``: ``labels``, the last step's native label map (``native_labels``; a
        pool's entry for the stream), when that step went the way back from the working size -- else (None) ``current_masks`` with the
        object LUT; ValueError when that answer has another size than the frame."""
        size = tuple(image.shape[-2:])
        if labels is not None and tuple(labels.shape[-2:]) == size:
            return labels.reshape(size), None
        masks = self.current_masks
        if labels is None and masks is not None and tuple(masks.shape[-2:]) == size and masks.shape[0] == len(self.targets) + 1:
            return masks.contiguous(), self._object_lut()
        raise ValueError('render: no answer for a frame of size %r (the last step answered at %s)'
                         % (size, 'no size: nothing was tracked' if masks is None and labels is None else
                            tuple((labels if labels is not None else masks).shape[-2:])))

    @torch.no_grad()
    def render(self, image, style=None, out=None):
        """The last answer of track() drawn onto its frame ``image`` (a (3, H, W) uint8 tensor or an ops.DecoderFrame) in one launch
        (ops.render_frames): ``style`` an ops.RenderStyle (default: the DAVIS palette at half opacity), ``out`` None (a new frame of the
        same kind and layout), ``image`` itself (in place) or the caller's surface.  -> the rendered frame."""
        answer, lut = self.render_answer(image, self.native_labels)
        return ops.render_frames([image], [answer], ops.default_render_style() if style is None else style, luts=[lut],
                                 out=None if out is None else [out])[0]

    def describe_answer(self, labels, planes=None):
        """(stack, lut) of ops.describe_frames for the last answer: ``current_masks`` -- or, when the last step went the way back from the
        working size (``labels``: its native label map, ``native_labels`` or a pool's entry for the stream), the native-size planes that
        step returned: ``planes`` when the caller kept them, else the ones _to_native keeps per shape -- with the object LUT."""
        masks = self.current_masks
        if masks is None:
            raise ValueError('describe: no answer (the last step answered at no size: nothing was tracked)')
        K = masks.shape[0]
        if K != len(self.targets) + 1:
            raise ValueError('describe: the last answer has %d planes, the tracker %d objects' % (K, len(self.targets)))
        if labels is None:
            return masks.contiguous(), self._object_lut()
        native = tuple(int(v) for v in labels.shape[-2:])
        if planes is None:
            kept = self._native_bufs.get((1, K, native, True))
            if kept is None:
                raise ValueError('describe: no answer of size %r with %d planes (the last step answered at %r)' % (native, K, tuple(masks.shape[-2:])))
            planes = kept[1].view(K, *native)
        return planes, self._object_lut()

    @torch.no_grad()
    def describe(self, out=None):
        """The objects of the last answer of track() measured in one launch (ops.describe_frames on the stack track() returned and the
        object LUT): -> an ops.ObjectReport of one frame; ``out``: a report whose buffer is used again."""
        stack, lut = self.describe_answer(self.native_labels)
        return ops.describe_frames([stack], luts=[lut], out=out)

    @torch.no_grad()
    def encode(self, out=None, capacity=None):
        """The objects of the last answer of track() as COCO run lengths, coded on the device (ops.encode_frames on the stack track() returned
        -- under ``working_size`` the native-size stack -- and the object LUT): -> an ops.MaskRuns of one frame; ``out``: a MaskRuns whose
        buffers are used again; ``capacity``: the elements of its ``runs`` (default: K (8 w + 8))."""
        stack, lut = self.describe_answer(self.native_labels)
        return ops.encode_frames([stack], luts=[lut], out=out, capacity=capacity)

    @torch.no_grad()
    def clean(self, out=None, **rule):
        """The last answer of track() cleaned on the device (ops.clean_frames on the stack track() returned -- under ``working_size`` the
        native-size stack -- and the object LUT): every object split into its connected parts and the rule applied; ``rule``:
        connectivity, min_area, largest_only, fill, components.  -> an ops.CleanedAnswers of one frame whose ``answers()`` go to
        ops.describe_frames / encode_frames / render_frames.  A post-process of the ANSWER: ``current_masks``, the target models' memory
        and every other state of the tracker stay as they are.  ``out``: a CleanedAnswers whose buffers are used again."""
        stack, lut = self.describe_answer(self.native_labels)
        plane_ids = (0,) + tuple(int(t.object_id) for t in sorted(self.targets.values(), key=lambda t: t.index))
        return ops.clean_frames([stack], luts=[lut], plane_ids=[plane_ids], out=out, **rule)

    def _track(self, image, features, im_size):
        if self._unchecked_fits and not self._in_run_sequence:
            self._check_first_frame_fits()
        if features is None:
            features = self.feature_extractor(image)
        active = self.active_targets()
        if self.fused_tail(active) and self.current_masks.is_contiguous():
            fused_step(self.refiner, [active], features, im_size, self.disc_params.update_filters, masks=self.current_masks)    # in place
        else:
            self._track_stepwise(active, features, im_size, 1, windowed=False)
        return self.current_masks
