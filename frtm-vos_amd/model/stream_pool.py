"""Several live streams on one GPU: ``StreamPool`` batches the per-frame work of S independent trackers ACROSS streams.

A camera or a call delivers one frame at a time, so only the literal ``Tracker.track(image)`` loop can serve it, and that loop is bound by
the batch-1 trunk (2.1 ms for one frame, 0.9 ms per frame in a batch of 8).  A server with several live streams does not need a faster
batch-1 trunk: every stream delivers one frame per tick, so the frames of all streams share ONE trunk pass, and the streams with the same
number of objects share one refiner pass and one merge (and, with ``grouped_apply``, one grouped target-model launch,
ops.target_apply_grouped).  Each stream keeps its own target models and memory: per stream the arithmetic is that of ``track()``.  The
reference has no such API.  A group runs the step that ``track()`` and ``track_window()`` run: ``fused_step`` of
model/tracker.py, with one list of target models per stream.  With ``ragged_groups`` the streams of a frame size share that pass whatever
their object counts (plan_tick_ragged; the indexed kernels of csrc/ragged_group.hip).

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
from .tracker import FrameTaps, Tracker, fused_step, persistent_taps

TickBatch = namedtuple('TickBatch', 'size order groups fallbacks')
TickPlan = namedtuple('TickPlan', 'batches skipped')


def plan_tick(entries, working_size=None):
    """The plan of one tick, a pure function of ``entries`` = (sid, frame size, number of active objects, eligible) per stream named.

    -> TickPlan(batches, skipped).  One TickBatch per frame size (sizes in ascending order): ``order`` = the sids in trunk-batch order,
    ``groups`` = (start, g, n): the g streams order[start:start + g] have n active objects each and take the fused step together --
    contiguous in batch order, so their taps are one slice --, ``fallbacks`` = the batch indices of the streams that run their own
    ``track()`` on their slice of the taps (ineligible: an object starts on this frame, host-side guards, a raw log).  ``skipped`` =
    streams without an active object: they take no part in the tick.  The result does not depend on the order of ``entries``.
    ``working_size``: every stream is tracked at this size whatever the size of its frames, so all streams form ONE TickBatch."""
    by_size, skipped = {}, []
    for sid, size, n, eligible in entries:
        size = size if working_size is None else working_size
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


def plan_tick_ragged(entries, working_size=None):
    """plan_tick for a pool with ``ragged_groups``: the same batches, order, fallbacks and skipped streams, but ONE group per frame size,
    (start, g, counts): ALL eligible streams of the size, order[start:start + g], take the fused step together whatever their object
    counts -- counts[i] active objects on stream i of the group, ascending, since the order is by count and then by sid.  A stream with
    more than 15 active objects (the merge kernel's bound, ops.MAX_MERGE_OBJECTS) is a fallback.  Pure, and independent of the order of
    ``entries``, like plan_tick; ``working_size`` as there."""
    by_size, skipped = {}, []
    for sid, size, n, eligible in entries:
        size = size if working_size is None else working_size
        if n <= 0:
            skipped.append(sid)
            continue
        eligible = bool(eligible) and int(n) <= ops.MAX_MERGE_OBJECTS
        by_size.setdefault(tuple(size), []).append((not eligible, int(n) if eligible else 0, sid))
    batches = []
    for size in sorted(by_size):
        rows = sorted(by_size[size])                       # eligible streams first, by object count; then the fallbacks; by sid within
        g = sum(1 for r in rows if not r[0])
        groups = [(0, g, tuple(r[1] for r in rows[:g]))] if g else []
        batches.append(TickBatch(size, [sid for _, _, sid in rows], groups, list(range(g, len(rows)))))
    return TickPlan(batches, sorted(skipped))


class _Stream:
    def __init__(self, tracker):
        self.tracker = tracker
        self.pool_masks = False         # tracker.current_masks is a view of one of the pool's merge buffers


class StreamPool:

    def __init__(self, augmenter, feature_extractor, disc_params, refiner, device, max_streams=8, grouped_apply=False, min_pairs=2,
                 trunk_lanes=2, ragged_groups=False, working_size=None):
        """One augmenter, one trunk and one refiner for up to ``max_streams`` per-stream Tracker states built over those same modules.
        grouped_apply  True: the groups' target models score through ONE ops.target_apply_grouped launch pair; False: per pair
                       ``Discriminator.apply(ft, interleave=...)`` (three small launches each) -- the A/B of tools/stream_pool_time.py.
                       Default False, by the rule of the bf16x1 routers: measured at 480x854 / RN101 / 2 objects per stream
                       (profiles/stream_pool_time.txt) the grouped arm's median tick is shorter from 4 pairs on (-0.09 ms of 4.73 at 4
                       pairs, -0.42 of 11.70 at 16, -0.68 of 21.88 at 32), but at no measured pair count by more than the per-pair
                       arm's own max - min over its 24 ticks (0.21 / 0.77 / 1.06 ms).
        min_pairs      pair count (streams x objects of a group) from which the grouped launch is used when grouped_apply is on.  The
                       measurement names no count (see above), so the starting value 2 stands: one pair gains nothing from grouping
                       (measured at 2 pairs: +0.02 ms).
        ragged_groups  True: all eligible streams of one frame size take the fused step together whatever their object counts
                       (plan_tick_ragged): one refiner pass, one merge and, with grouped_apply, one grouped scoring launch per frame size
                       and tick, on the indexed kernels of csrc/ragged_group.hip; a group whose counts are all equal runs exactly as
                       without the option.  False (default): streams share a pass only when their object counts are equal (plan_tick) -- same
                       launches, same bits as before the option existed.  Measured at 480x854 / RN101 (profiles/stream_pool_ragged_time.txt):
                       8 streams with 1, 1, 2, 2, 3, 3, 4 and 5 objects 14.59 -> 12.68 ms per tick against a max - min of 0.33 ms, 4 streams
                       with 1 .. 4 objects 8.87 -> 7.16 ms, nothing on equal counts; one measurement introduces the option, the default waits.
        working_size   (h, w): every stream is tracked at this size whatever the size of its frames (Tracker's option of that name), so ALL
                       streams of a tick share one trunk pass and the group rules above: the frames are packed into one staging buffer and
                       resized by one launch (csrc/frame_resize.hip), and each group's masks go back to every stream's native size in one
                       launch (ops.masks_to_native).  step() then answers at native size; the streams' state stays at the working size.
                       None (default): one trunk pass per frame size -- same launches, same bits as before the option existed."""
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
        self.ragged_groups = bool(ragged_groups)
        self.working_size = None if working_size is None else (int(working_size[0]), int(working_size[1]))
        self._streams = {}
        self._next_sid = 0
        self._disc_pool = []            # released target models, shared by all streams (Tracker.release_targets)
        self._bufs = {}                 # (kind, g, n, size) or (kind, counts, size) -> preallocated device tensor
        self._tables = {}               # (g, n, size) or (counts, size) -> apply_grouped's table cache of the group that last ran under this key
        self._ragged = {}               # (counts, size) -> ops.RaggedTable: one table for the scoring, the refiner and the merge
        self.grouped_launches = 0       # ops.target_apply_grouped calls so far (diagnostics)
        self.refiner_passes = 0         # refiner calls made by groups so far (diagnostics)
        self.trunk_passes = 0           # trunk calls made by step() so far (diagnostics)
        self.frame_launches = 0         # ops.FramePlan launches made by step() so far: one per TickBatch that holds a DecoderFrame (diagnostics)
        self.render_launches = 0        # ops.render_frames launches made by render() so far: one per call (diagnostics)
        self._frame_plans = {}          # layouts of a tick's batch, in order -> (ops.FramePlan, staging buffer, byte offsets and counts)
        self._plans = {}                # native sizes of a tick's batch, in order -> (ops.ResizePlan, staging buffer, byte offsets)
        self._native = {}               # (group key, native sizes) -> [ops.NativeTable, labels, soft, object ids of the rows, their LUTs]
        # sid -> (H, W) uint8 label map (object ids, as Tracker.native_labels) at native size, for the streams whose LAST step went the way back
        # from the working size; a stream whose last step answered with its current_masks (frame at the working size, or no option) has no entry
        self.native_labels = {}
        # sid -> (that label map, the stream's (K, H, W) native planes of the same group launch): describe() reads the planes while the entry's
        # label map is still the stream's ``native_labels`` entry (a later step of another kind leaves this entry behind, and it is ignored)
        self._native_planes = {}
        self.describe_launches = 0      # ops.describe_frames launches made by describe() so far: one per call (diagnostics)
        self.encode_launches = 0        # ops.encode_frames launches made by encode() so far: one per call (diagnostics)
        self.clean_launches = 0         # ops.clean_frames calls made by clean() so far: one per call (diagnostics)

    # ---- streams ------------------------------------------------------------------------------------------------------------
    def open(self):
        if len(self._streams) >= self.max_streams:
            raise RuntimeError('StreamPool: %d streams are open already (max_streams)' % self.max_streams)
        tr = Tracker(self.augmenter, self.feature_extractor, self.disc_params, self.refiner, self.device, working_size=self.working_size)
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
        """Tracker.initialize for stream ``sid``: the first frame, or objects that appear later; before step() on that frame.  ``image``:
        a (3,H,W) uint8 tensor or an ops.DecoderFrame."""
        st = self._streams[sid]
        if not isinstance(image, ops.DecoderFrame):
            image = image.to(self.device)
        out = st.tracker.initialize(image, labels.to(self.device), new_objects)
        st.pool_masks = False                           # (initialize() gives the stream a mask stack of its own)
        return out

    # ---- one tick -----------------------------------------------------------------------------------------------------------
    def _eligible(self, tr, active):
        """Does this stream's frame take the fused step (Tracker.fused_tail), with every early-out decided on the device?"""
        return tr.fused_tail(active) and (not self.disc_params.update_filters or all(t.discriminator.guards_on_device() for t in active))

    def _buf(self, kind, key, shape, dtype=torch.float32):
        b = self._bufs.get((kind,) + key)
        if b is None:
            b = self._bufs[(kind,) + key] = torch.empty(shape, dtype=dtype, device=self.device)
        return b

    @torch.no_grad()
    def step(self, frames):
        """Tracks one frame for every stream named: {sid: image (3,H,W) uint8 or ops.DecoderFrame} -> {sid: masks (n_obj + 1, H, W)}.  A stream without an
        active object (no target yet, or all of them start on this very frame) is skipped and absent from the result.  Every stream's
        current_frame advances by one.  The masks are the streams' ``current_masks``: valid until that stream's next step, like track()'s.
        Under ``working_size`` a stream whose frame has another size gets its masks at the frame's NATIVE size instead, from a buffer the
        pool keeps (valid until that stream's next step as well; its label map in ``native_labels[sid]``), while its ``current_masks``
        stays at the working size."""
        for sid in frames:
            if sid not in self._streams:
                raise KeyError(sid)
        for sid in frames:
            self.native_labels.pop(sid, None)
        entries, active_of = [], {}
        for sid, image in frames.items():
            tr = self._streams[sid].tracker
            if tr._unchecked_fits:
                tr._check_first_frame_fits()            # as track(): no frame is scored with a half-fitted model
            active = active_of[sid] = tr.active_targets()
            entries.append((sid, tuple(image.shape[-2:]), len(active), self._eligible(tr, active)))
        plan = (plan_tick_ragged if self.ragged_groups else plan_tick)(entries, working_size=self.working_size)
        out = {}
        ext = self.feature_extractor
        for tb in plan.batches:
            for k in tb.fallbacks:
                st = self._streams[tb.order[k]]
                if st.pool_masks:
                    # its mask stack is a row of a merge buffer that a group of this tick may write; track() works in place: on a copy
                    st.tracker.current_masks = st.tracker.current_masks.clone()
                    st.pool_masks = False
        with persistent_taps(ext, max(1, self.trunk_lanes), False, [(ext, 'output_set', 0)]):
            for tb in plan.batches:
                B = len(tb.order)
                batch = self._buf('frames', (B, 3, tb.size), (B, 3) + tb.size, torch.uint8)
                natives = tuple(tuple(frames[sid].shape[-2:]) for sid in tb.order)
                if any(isinstance(frames[sid], ops.DecoderFrame) for sid in tb.order):
                    self._convert_batch(tb, frames, batch)
                elif any(nat != tb.size for nat in natives):            # (only under working_size)
                    self._resize_batch(tb, natives, frames, batch)
                else:
                    for k, sid in enumerate(tb.order):
                        batch[k].copy_(frames[sid], non_blocking=True)
                taps = ext(batch)                                       # ONE trunk pass for the streams of this size
                self.trunk_passes += 1
                for start, g, n in tb.groups:
                    self._run_group(tb, start, g, n, taps, active_of, out, natives)
                for k in tb.fallbacks:
                    sid = tb.order[k]
                    tr = self._streams[sid].tracker
                    out[sid] = tr.track(batch[k], features=FrameTaps(taps, k))
                    if natives[k] != tb.size:                           # its own way back, like Tracker.track on a native frame
                        labels, soft = tr._to_native(tr.current_masks.unsqueeze(0), natives[k], tr._object_lut(), soft=True, keep=True)
                        tr.native_labels, out[sid] = labels[0], soft[0]
                        self.native_labels[sid] = labels[0, 0]
                del taps                                                # no tap view outlives the tick: the next pass overwrites them
        for sid in frames:
            self._streams[sid].tracker.current_frame += 1
        return out

    @torch.no_grad()
    def render(self, frames, style=None, out=None):
        """The last answer of every stream named drawn onto its frame: {sid: image (3,H,W) uint8 or ops.DecoderFrame} -> {sid: rendered
        frame}, ONE ops.render_frames launch for all of them whatever their sizes and formats.  A stream whose last step went the way
        back from the working size is drawn from ``native_labels[sid]``, every other one from its ``current_masks`` and object LUT;
        ValueError when that answer has another size than the frame.  ``style``: an ops.RenderStyle (default: the DAVIS palette at half
        opacity); ``out``: None (new frames of the same kind and layout), ``frames`` itself (in place) or {sid: the caller's surface}."""
        sids = list(frames)
        if not sids:
            return {}
        if out is not None and sorted(out, key=repr) != sorted(sids, key=repr):
            raise KeyError('StreamPool.render: out names other streams than frames')
        answers, luts = [], []
        for sid in sids:
            answer, lut = self._streams[sid].tracker.render_answer(frames[sid], self.native_labels.get(sid))
            answers.append(answer)
            luts.append(lut)
        done = ops.render_frames([frames[sid] for sid in sids], answers, ops.default_render_style() if style is None else style, luts=luts,
                                 out=None if out is None else [out[sid] for sid in sids])
        self.render_launches += 1
        return dict(zip(sids, done))

    def _answers(self, who, sids):
        """(sids, stacks, luts) of the last answers of the streams named (None: every stream that has one), for describe() and encode()."""
        if sids is None:
            sids = [sid for sid, st in self._streams.items() if st.tracker.current_masks is not None]
        sids = list(sids)
        if not sids:
            raise ValueError('StreamPool.%s: no stream has an answer (nothing was tracked)' % who)
        stacks, luts = [], []
        for sid in sids:
            labels = self.native_labels.get(sid)
            kept = self._native_planes.get(sid)
            stack, lut = self._streams[sid].tracker.describe_answer(labels, kept[1] if kept is not None and kept[0] is labels else None)
            stacks.append(stack)
            luts.append(lut)
        return sids, stacks, luts

    @torch.no_grad()
    def describe(self, sids=None, out=None):
        """The objects of the last answer of every stream named measured -- area, box, centroid sums, edge and border pixels, confidence,
        soft area --: -> ({sid: index}, ops.ObjectReport), ONE ops.describe_frames launch for all of them whatever their sizes and object
        counts.  ``sids``: None -- every stream that has an answer -- or the streams to measure.  Every stream is measured on the stack its
        last step returned (its ``current_masks``, or its native-size planes when that step went the way back from the working size) with
        its object LUT.  ``out``: a report whose buffer is used again."""
        sids, stacks, luts = self._answers('describe', sids)
        report = ops.describe_frames(stacks, luts=luts, out=out)
        self.describe_launches += 1
        return {sid: i for i, sid in enumerate(sids)}, report

    @torch.no_grad()
    def encode(self, sids=None, out=None, capacity=None):
        """The objects of the last answer of every stream named as COCO run lengths, coded on the device: -> ({sid: index}, ops.MaskRuns),
        ONE ops.encode_frames call for all of them whatever their sizes and object counts.  ``sids`` and the stack every stream is coded
        from: describe()'s.  ``out``: a MaskRuns whose buffers are used again; ``capacity``: the elements of its ``runs``."""
        sids, stacks, luts = self._answers('encode', sids)
        coded = ops.encode_frames(stacks, luts=luts, out=out, capacity=capacity)
        self.encode_launches += 1
        return {sid: i for i, sid in enumerate(sids)}, coded

    @torch.no_grad()
    def clean(self, sids=None, out=None, **rule):
        """The last answer of every stream named cleaned on the device -- every object split into its connected parts, specks dropped by
        ``rule`` (connectivity, min_area, largest_only, fill, components) --: -> ({sid: index}, ops.CleanedAnswers), ONE ops.clean_frames
        call for all of them whatever their sizes and object counts.  ``sids`` and the stack every stream is cleaned from: describe()'s.
        A post-process of the answers: no stream's ``current_masks``, memory or label map is written.  ``out``: a CleanedAnswers whose
        buffers are used again."""
        sids, stacks, luts = self._answers('clean', sids)
        plane_ids = [(0,) + tuple(int(t.object_id) for t in sorted(self._streams[sid].tracker.targets.values(), key=lambda t: t.index))
                     for sid in sids]
        cleaned = ops.clean_frames(stacks, luts=luts, plane_ids=plane_ids, out=out, **rule)
        self.clean_launches += 1
        return {sid: i for i, sid in enumerate(sids)}, cleaned

    def _resize_batch(self, tb, natives, frames, batch):
        """The tick's frames, of any sizes, into ``batch`` (B,3,h,w) at the working size: copied into ONE packed staging buffer (16-byte
        aligned offsets) and resized by ONE launch, mode 'area' (the identity, bit for bit, for a frame that has the working size)."""
        plan = self._plans.get(natives)
        if plan is None:
            offs, o = [], 0
            for Hn, Wn in natives:
                offs.append(o)
                o += (3 * Hn * Wn + 15) // 16 * 16
            desc = torch.tensor([[offs[k], nat[0], nat[1], ops.RESIZE_MODES['area']] for k, nat in enumerate(natives)], dtype=torch.int64)
            plan = self._plans[natives] = (ops.ResizePlan(desc, self.device), torch.empty(o, dtype=torch.uint8, device=self.device), offs)
        rp, staging, offs = plan
        for k, sid in enumerate(tb.order):
            Hn, Wn = natives[k]
            if frames[sid].dtype != torch.uint8:
                raise TypeError('StreamPool: working_size resizes uint8 frames, got %s' % frames[sid].dtype)
            staging[offs[k]:offs[k] + 3 * Hn * Wn].view(3, Hn, Wn).copy_(frames[sid], non_blocking=True)
        rp.frames(staging, 3, tb.size, out=batch)

    def _convert_batch(self, tb, frames, batch):
        """_resize_batch for a tick that holds at least one ops.DecoderFrame, with or without a working size: every frame's bytes -- a
        tensor's 3 h w, a decoder frame's nbytes_needed -- into ONE packed staging buffer (16-byte aligned offsets), and ONE ops.FramePlan
        launch converts the NV12 rows, passes the planar ones on (format 'rgb') and takes all of them to the batch's size, mode 'area'."""
        key = tuple(f.plan_key() if isinstance(f, ops.DecoderFrame) else tuple(f.shape[-2:]) for f in (frames[sid] for sid in tb.order))
        plan = self._frame_plans.get(key)
        if plan is None:
            rows, spans, o = [], [], 0
            for sid in tb.order:
                f = frames[sid]
                if isinstance(f, ops.DecoderFrame):
                    rows.append(f.row(o, 'area'))
                    nbytes = f.nbytes_needed
                else:
                    Hn, Wn = f.shape[-2:]
                    rows.append([o, Hn, Wn, ops.RESIZE_MODES['area'], ops.FRAME_FORMATS['rgb'], 0, 0, 0])
                    nbytes = 3 * Hn * Wn
                spans.append((o, nbytes))
                o += (nbytes + 15) // 16 * 16
            plan = self._frame_plans[key] = (ops.FramePlan(torch.tensor(rows, dtype=torch.int64), self.device),
                                             torch.empty(o, dtype=torch.uint8, device=self.device), spans)
        fp, staging, spans = plan
        for (o, nbytes), sid in zip(spans, tb.order):
            f = frames[sid]
            if isinstance(f, ops.DecoderFrame):
                staging[o:o + nbytes].copy_(f.data[:nbytes], non_blocking=True)
            else:
                if f.dtype != torch.uint8:
                    raise TypeError('StreamPool: a tick with decoder frames converts uint8 frames, got %s' % f.dtype)
                staging[o:o + nbytes].view(f.shape[-3:]).copy_(f, non_blocking=True)
        fp.frames(staging, tb.size, out=batch)
        self.frame_launches += 1

    def _group_to_native(self, key, masks, sids, planes, natives, size, out):
        """The streams of a group whose frames have another size than the working size get their masks at native size: ONE
        ops.masks_to_native launch for the group, into buffers kept per (group, native sizes); ``planes[i]``: (first plane, K) of stream
        i in ``masks``.  The streams' state (current_masks) stays at the working size."""
        rows_of = [i for i in range(len(sids)) if natives[i] != size]
        if not rows_of:
            return
        nkey = (key, tuple(natives))
        ent = self._native.get(nkey)
        if ent is None:
            rows, lo, so, to = [], 0, 0, 0
            for i in rows_of:
                (a, K), (Hn, Wn) = planes[i], natives[i]
                rows.append((a * size[0] * size[1], K, Hn, Wn, lo, so, to))
                lo, so, to = lo + Hn * Wn, so + K * Hn * Wn, to + K
            table = ops.NativeTable(rows, self.device)
            ent = self._native[nkey] = [table, torch.empty(table.label_bytes, dtype=torch.uint8, device=self.device),
                                        torch.empty(table.soft_elems, device=self.device), None, None]
        # every row's LUT: plane -> object id of ITS stream (Tracker._object_lut's ids); uploaded again only when a stream's objects change
        ids = tuple(i_ for i in rows_of for i_ in self._plane_ids(sids[i], planes[i][1]))
        if ent[3] != ids:
            ent[3], ent[4] = ids, H.upload(torch.tensor(ids, dtype=torch.uint8), self.device)
        table, labels, soft, _, luts = ent
        ops.masks_to_native(masks, table, labels, luts, soft=soft)
        for r, i in enumerate(rows_of):
            out[sids[i]] = table.soft_of(soft, r)
            self.native_labels[sids[i]] = table.labels_of(labels, r)
            self._native_planes[sids[i]] = (self.native_labels[sids[i]], out[sids[i]])

    def _plane_ids(self, sid, K):
        """Object id of each of stream ``sid``'s K mask planes (plane 0: the background, id 0)."""
        tr = self._streams[sid].tracker
        tr._object_lut()                                # (refuses ids beyond 255)
        ids = (0,) + tr._native_lut[0]
        if len(ids) != K:
            raise RuntimeError('StreamPool: stream %r has %d mask planes and %d objects' % (sid, K, len(ids) - 1))
        return ids

    def _run_group(self, tb, start, g, n, taps, active_of, out, natives=None):
        """The fused step (model/tracker.py: fused_step) for g streams of n objects at once, one frame each, on the pool's buffers:
        pair p = i * n + k is (stream i of the group, its object k).  n a tuple (plan_tick_ragged): stream i carries n[i] objects."""
        self.refiner_passes += 1
        if isinstance(n, tuple):
            if len(set(n)) > 1:
                return self._run_ragged_group(tb, start, n, taps, active_of, out, natives)
            n = n[0]                                    # equal counts: exactly the uniform group
        key = (g, n, tb.size)
        sids = tb.order[start:start + g]
        first = active_of[sids[0]][0]
        feats = {L: t[start:start + g] for L, t in taps.items()}
        h_, w_ = feats[first.disc_layer].shape[-2:]
        P = g * n
        grouped = None
        if self.grouped_apply and P >= self.min_pairs:
            grouped = (self._tables.setdefault(key, {}), self._buf('cft', key, (P, first.discriminator.project.out_channels, h_, w_)))
            self.grouped_launches += 1
        update = bool(self.disc_params.update_filters)
        masks, _ = fused_step(self.refiner, [active_of[sid] for sid in sids], feats, tb.size, update,
                              scores=self._buf('scores', key, (P, 1, h_, w_)), masks=self._buf('masks', key, (g, n + 1) + tb.size),
                              counts=self._buf('counts', key, (g, n + 1), torch.int32) if update else None, grouped=grouped)
        for i, sid in enumerate(sids):
            st = self._streams[sid]
            st.tracker.current_masks = masks[i]
            st.pool_masks = True
            out[sid] = masks[i]
        if natives is not None and self.working_size is not None:
            self._group_to_native(key, masks, sids, [(i * (n + 1), n + 1) for i in range(g)], natives[start:start + g], tb.size, out)

    def _run_ragged_group(self, tb, start, counts, taps, active_of, out, natives=None):
        """_run_group for streams with different object counts: pairs stream-major, stream i's masks the planes table.planes(i) of ONE
        packed merge buffer.  Buffers and tables are kept per (counts, size): steady ticks allocate nothing."""
        key = (counts, tb.size)
        g = len(counts)
        sids = tb.order[start:start + g]
        first = active_of[sids[0]][0]
        feats = {L: t[start:start + g] for L, t in taps.items()}
        h_, w_ = feats[first.disc_layer].shape[-2:]
        table = self._ragged.get(key)
        if table is None:
            table = self._ragged[key] = ops.RaggedTable(counts, self.device)
        P = table.n
        grouped = None
        if self.grouped_apply and P >= self.min_pairs:
            grouped = (self._tables.setdefault(key, {}), self._buf('cft', key, (P, first.discriminator.project.out_channels, h_, w_)))
            self.grouped_launches += 1
        update = bool(self.disc_params.update_filters)
        masks, _ = fused_step(self.refiner, [active_of[sid] for sid in sids], feats, tb.size, update,
                              scores=self._buf('scores', key, (P, 1, h_, w_)), masks=self._buf('masks', key, (P + g,) + tb.size),
                              counts=self._buf('counts', key, (P + g,), torch.int32) if update else None, grouped=grouped, table=table)
        for i, sid in enumerate(sids):
            st = self._streams[sid]
            a, b = table.planes(i)
            st.tracker.current_masks = masks[a:b]
            st.pool_masks = True
            out[sid] = masks[a:b]
        if natives is not None and self.working_size is not None:
            self._group_to_native(key, masks, sids, [(table.planes(i)[0], counts[i]  + 1) for i in range(g)], natives[start:start + g], tb.size, out)
