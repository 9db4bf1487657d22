"""Several live streams on one GPU: ``StreamPool`` batches the per-frame work of S independent trackers ACROSS streams.

A camera or a call delivers one frame at a time, so only the literal ``Tracker.track(image)`` loop can serve it, and that loop is bound by
the batch-1 trunk (2.1 ms for one frame, 0.9 ms per frame in a batch of 8).  A server with several live streams does not need a faster
batch-1 trunk: every stream delivers one frame per tick, so the frames of all streams share ONE trunk pass, and the streams with the same
number of objects share one refiner pass and one merge (and, with ``grouped_apply``, one grouped target-model launch,
ops.target_apply_grouped).  Each stream keeps its own target models and memory: per stream the arithmetic is that of ``track()``.  The
reference has no such API.

    pool = Parameters(weights).get_stream_pool(max_streams=8)
    sid = pool.open()
    pool.initialize(sid, image, labels, new_objects)      # first frame / late objects, BEFORE step() on that frame
    masks = pool.step({sid: image, ...})[sid]             # (n_obj + 1, H, W), as track() returns it
    pool.close(sid)
"""
from collections import namedtuple

import torch

from .. import _hip as H
from .. import ops
from .tracker import FrameTaps, Tracker

TickBatch = namedtuple('TickBatch', 'size order groups fallbacks')
TickPlan = namedtuple('TickPlan', 'batches skipped')


def plan_tick(entries):
    """The plan of one tick, a pure function of ``entries`` = (sid, frame size, number of active objects, eligible) per stream named.

    -> TickPlan(batches, skipped).  One TickBatch per frame size (sizes in ascending order): ``order`` = the sids in trunk-batch order,
    ``groups`` = (start, g, n): the g streams order[start:start + g] have n active objects each and take the fused branch together --
    contiguous in batch order, so their taps are one slice --, ``fallbacks`` = the batch indices of the streams that run their own
    ``track()`` on their slice of the taps (ineligible: an object starts on this frame, host-side guards, a raw log).  ``skipped`` =
    streams without an active object: they take no part in the tick.  The result does not depend on the order of ``entries``."""
    by_size, skipped = {}, []
    for sid, size, n, eligible in entries:
        if n <= 0:
            skipped.append(sid)
            continue
        by_size.setdefault(tuple(size), []).append((not eligible, int(n) if eligible else 0, sid))
    batches = []
    for size in sorted(by_size):
        rows = sorted(by_size[size])                       # eligible streams first, by object count; then the fallbacks; by sid within
        order = [sid for _, _, sid in rows]
        groups, fallbacks, k = [], [], 0
        while k < len(rows):
            if rows[k][0]:
                fallbacks.append(k)
                k += 1
                continue
            g = 1
            while k + g < len(rows) and not rows[k + g][0] and rows[k + g][1] == rows[k][1]:
                g += 1
            groups.append((k, g, rows[k][1]))
            k += g
        batches.append(TickBatch(size, order, groups, fallbacks))
    return TickPlan(batches, sorted(skipped))


class _Stream:
    def __init__(self, tracker):
        self.tracker = tracker
        self.pool_masks = False         # tracker.current_masks is a view of one of the pool's merge buffers


class StreamPool:

    def __init__(self, augmenter, feature_extractor, disc_params, refiner, device, max_streams=8, grouped_apply=False, min_pairs=2,
                 trunk_lanes=2):
        """One augmenter, one trunk and one refiner for up to ``max_streams`` per-stream Tracker states built over those same modules.
        grouped_apply  True: the groups' target models score through ONE ops.target_apply_grouped launch pair; False: per pair
                       ``Discriminator.apply(ft, interleave=...)`` (three small launches each) -- the A/B of tools/stream_pool_time.py.
                       Default False, by the rule of the bf16x1 routers: measured at 480x854 / RN101 / 2 objects per stream
                       (profiles/stream_pool_time.txt) the grouped arm's median tick is shorter from 4 pairs on (-0.09 ms of 4.73 at 4
                       pairs, -0.42 of 11.70 at 16, -0.68 of 21.88 at 32), but at no measured pair count by more than the per-pair
                       arm's own max - min over its 24 ticks (0.21 / 0.77 / 1.06 ms).
        min_pairs      pair count (streams x objects of a group) from which the grouped launch is used when grouped_apply is on.  The
                       measurement names no count (see above), so the starting value 2 stands: one pair gains nothing from grouping
                       (measured at 2 pairs: +0.02 ms)."""
        if torch.device(device).type != 'cuda':
            raise RuntimeError('StreamPool: device %s; the FRTM hot path runs on the GPU only (no CPU fallback)' % (device,))
        if int(max_streams) < 1:
            raise ValueError('max_streams must be at least 1')
        self.device = H.normalize_device(device)
        self.augmenter, self.feature_extractor, self.disc_params, self.refiner = augmenter, feature_extractor, disc_params, refiner
        self.max_streams = int(max_streams)
        self.grouped_apply = bool(grouped_apply)
        self.min_pairs = int(min_pairs)
        self.trunk_lanes = int(trunk_lanes)
        self._streams = {}
        self._next_sid = 0
        self._disc_pool = []            # released target models, shared by all streams (Tracker.release_targets)
        self._bufs = {}                 # (kind, g, n, size) -> preallocated device tensor
        self._tables = {}               # (g, n, size) -> pointer tables of the group that last ran under this key
        self.grouped_launches = 0       # ops.target_apply_grouped calls so far (diagnostics)

    # ---- streams ------------------------------------------------------------------------------------------------------------
    def open(self):
        if len(self._streams) >= self.max_streams:
            raise RuntimeError('StreamPool: %d streams are open already (max_streams)' % self.max_streams)
        tr = Tracker(self.augmenter, self.feature_extractor, self.disc_params, self.refiner, self.device)
        tr.eval()
        tr._disc_pool = self._disc_pool                 # one pool of recycled target models for all streams
        sid, self._next_sid = self._next_sid, self._next_sid + 1
        self._streams[sid] = _Stream(tr)
        return sid

    def close(self, sid):
        st = self._streams.pop(sid)                     # KeyError: unknown stream
        st.tracker.release_targets()                    # the target models serve the next stream's objects: nothing is freed
        st.tracker.clear()

    def tracker(self, sid):
        """The stream's Tracker state (targets, current_frame, current_masks)."""
        return self._streams[sid].tracker

    def __len__(self):
        return len(self._streams)

    @torch.no_grad()
    def initialize(self, sid, image, labels, new_objects):
        """Tracker.initialize for stream ``sid``: the first frame, or objects that appear later; before step() on that frame."""
        st = self._streams[sid]
        out = st.tracker.initialize(image.to(self.device), labels.to(self.device), new_objects)
        st.pool_masks = False                           # (initialize() gives the stream a mask stack of its own)
        return out

    # ---- one tick -----------------------------------------------------------------------------------------------------------
    def _eligible(self, tr, active):
        """Would track() take its fused branch for this stream, with every early-out decided on the device?"""
        n = len(active)
        if not (tr.fuse_merge and active and n == len(tr.targets) and n < 16 and getattr(tr, '_raw_log', None) is None
                and all(t.index == k + 1 for k, t in enumerate(active))):
            return False
        if not self.disc_params.update_filters:
            return True
        return all(t.discriminator.guards_on_device() for t in active)

    def _buf(self, kind, key, shape, dtype=torch.float32):
        b = self._bufs.get((kind,) + key)
        if b is None:
            b = self._bufs[(kind,) + key] = torch.empty(shape, dtype=dtype, device=self.device)
        return b

    @torch.no_grad()
    def step(self, frames):
        """Tracks one frame for every stream named: {sid: image (3,H,W) uint8} -> {sid: masks (n_obj + 1, H, W)}.  A stream without an
        active object (no target yet, or all of them start on this very frame) is skipped and absent from the result.  Every stream's
        current_frame advances by one.  The masks are the streams' ``current_masks``: valid until that stream's next step, like track()'s."""
        for sid in frames:
            if sid not in self._streams:
                raise KeyError(sid)
        entries, active_of = [], {}
        for sid, image in frames.items():
            tr = self._streams[sid].tracker
            if getattr(tr, '_unchecked_fits', None):
                tr._check_first_frame_fits()            # as track(): no frame is scored with a half-fitted model
            active = [t for t in tr.targets.values() if t.start_frame < tr.current_frame]
            active_of[sid] = active
            entries.append((sid, tuple(image.shape[-2:]), len(active), self._eligible(tr, active)))
        plan = plan_tick(entries)
        out = {}
        ext = self.feature_extractor
        persistent = hasattr(ext, 'reuse_outputs')
        if persistent:
            saved = (ext.reuse_outputs, ext.use_graph, ext.output_set)
            ext.reuse_outputs, ext.use_graph, ext.output_set = True, False, 0
            if ext.lanes != max(1, self.trunk_lanes):
                ext.lanes = max(1, self.trunk_lanes)
        for tb in plan.batches:
            for k in tb.fallbacks:
                st = self._streams[tb.order[k]]
                if st.pool_masks:
                    # its mask stack is a row of a merge buffer that a group of this tick may write; track() works in place: on a copy
                    st.tracker.current_masks = st.tracker.current_masks.clone()
                    st.pool_masks = False
        try:
            for tb in plan.batches:
                B = len(tb.order)
                batch = self._buf('frames', (B, 3, tb.size), (B, 3) + tb.size, torch.uint8)
                for k, sid in enumerate(tb.order):
                    batch[k].copy_(frames[sid], non_blocking=True)
                taps = ext(batch)                                       # ONE trunk pass for the streams of this size
                for start, g, n in tb.groups:
                    self._run_group(tb, start, g, n, taps, active_of, out)
                for k in tb.fallbacks:
                    sid = tb.order[k]
                    out[sid] = self._streams[sid].tracker.track(batch[k], features=FrameTaps(taps, k))
                del taps                                                # no tap view outlives the tick: the next pass overwrites them
        finally:
            if persistent:
                ext.reuse_outputs, ext.use_graph, ext.output_set = saved
        for sid in frames:
            self._streams[sid].tracker.current_frame += 1
        return out

    def _run_group(self, tb, start, g, n, taps, active_of, out):
        """The fused branch of track() for g streams of n objects at once: pair p = i * n + k is (stream i of the group, its object k)."""
        key = (g, n, tb.size)
        sids = tb.order[start:start + g]
        discs = [t.discriminator for sid in sids for t in active_of[sid]]
        layer = active_of[sids[0]][0].disc_layer
        feats = {L: t[start:start + g] for L, t in taps.items()}
        ft = feats[layer]
        h_, w_ = ft.shape[-2:]
        P = g * n
        c = discs[0].project.out_channels
        scores = self._buf('scores', key, (P, 1, h_, w_))
        if self.grouped_apply and P >= self.min_pairs:
            w1T = [d._project_T() for d in discs]
            ptrs = [t.data_ptr() for t in w1T] + [d.filter.weight.data_ptr() for d in discs]
            tab = self._tables.get(key)
            if tab is None or tab['ptrs'] != ptrs:
                # membership of the group or one of the pointers changed (a filter re-solve writes in place: no change)
                tab = self._tables[key] = dict(ptrs=ptrs, w1T=ops.pointer_table(w1T, self.device),
                                               w2=ops.pointer_table([d.filter.weight.data for d in discs], self.device),
                                               frames=tab['frames'] if tab is not None else
                                               H.upload(torch.arange(P, dtype=torch.int32) // n, self.device))
            cft = self._buf('cft', key, (P, c, h_, w_))
            ops.target_apply_grouped(ft, tab['frames'], tab['w1T'], tab['w2'], c, cft=cft, scores=scores)
            self.grouped_launches += 1
            for p, d in enumerate(discs):
                d.advance(cft[p:p + 1])
        else:
            for p, d in enumerate(discs):
                d.apply(ft[p // n:p // n + 1], interleave=(scores, p, P))
        size = tb.size
        logits = self.refiner(scores, feats, size)                      # (g * n, 1, H, W), frame-major
        masks = self._buf('masks', key, (g, n + 1) + size)
        update = bool(self.disc_params.update_filters)
        counts = self._buf('counts', key, (g, n + 1), torch.int32) if update else None
        ops.track_merge(logits, g, n, masks, None, None, False, counts)
        for i, sid in enumerate(sids):
            st = self._streams[sid]
            if update:
                for t in active_of[sid]:
                    y = masks[i, t.index].unsqueeze(0).unsqueeze(0)
                    t.discriminator.update(y, count_dev=counts[i, t.index:t.index + 1])
            st.tracker.current_masks = masks[i]
            st.pool_masks = True
            out[sid] = masks[i]
