"""Thin tensor-level wrappers over the C ABI (include/frtm_hip.h).  Every function enqueues HIP
kernels on the current torch stream and returns torch tensors that own the device memory."""
import collections
import ctypes
import functools
import numbers

import torch

from . import _hip as H

_workspaces = {}


def workspace(device, elems):
    """Grow-only fp32 scratch (split-K partials) per device AND stream: convs enqueued on different streams may run
    concurrently and must not share partial sums.

    Inside a hipGraph capture the scratch is NOT taken from this process-wide cache: a tensor allocated while a capture is open comes
    from the capturing graph's private memory pool, and a cache entry allocated there outlives its pool -- the next tracker's graphs
    then baked in an address inside a pool that had been released with the previous tracker's refiner (the process aborted in a
    later replay, tools/graph_lifetime_check.py).  A capture gets a fresh allocation from its own pool instead, like every other
    intermediate of the captured sequence: the pool keeps it for the graph's lifetime."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(int(elems), device=device, dtype=torch.float32)
    key = (device, H.stream())
    w = _workspaces.get(key)
    if w is None or w.numel() < elems:
        w = torch.empty(int(elems), device=device, dtype=torch.float32)
        _workspaces[key] = w
    return w


def padded_rows(K):
    return (K + 31) // 32 * 32


def padded_cols(M):
    return (M + 31) // 32 * 32


def bf16x3_elems(Cout, Cin):
    """Floats of a FRTM_WLAYOUT_BF16X3 image (FRTM_CONV_BF16X3_ELEMS): three bf16 planes [Cin/8][Mp][8], Mp = Cout rounded up to 128."""
    return 3 * ((Cin + 15) // 16 * 16) * ((Cout + 127) // 128 * 128) // 2


def bf16x1_elems(Cout, Cin):
    """Floats of a FRTM_WLAYOUT_BF16X1 image (FRTM_CONV_BF16X1_ELEMS): one bf16 plane [Cin/8][Mp][8], Mp = Cout rounded up to 128."""
    return ((Cin + 15) // 16 * 16) * ((Cout + 127) // 128 * 128) // 2


def bf16x1_3x3_elems(Cout, Cin):
    """Floats of a FRTM_WLAYOUT_BF16X1_3X3 image (FRTM_CONV_BF16X1_3X3_ELEMS): bf16 [Cin/16][tap][2][Mp][8], Mp = Cout rounded up to 32."""
    return 9 * ((Cin + 15) // 16 * 16) * ((Cout + 31) // 32 * 32) // 2


def pack_weights(w_oihw, halo=None, wino=False, wino4=False, wino6=False, bf16x3=False, bf16x1=False, stride=1):
    """(Cout,Cin,k,k) -> packed GEMM weights (+ ktab for k > 1).  3x3 kernels default to the halo layout
    (valid for pad-1 convs of stride 1 or 2); wino=True: Winograd F(2x2,3x3) image (stride 1, pad 1); wino4=True: the 36 transformed
    weight matrices of Winograd F(4x4,3x3) (FRTM_WLAYOUT_WINO4; conv2d then needs ``ws`` = wino4_workspace(...)); wino6=True: the 64 of
    F(6x6,3x3) (FRTM_WLAYOUT_WINO6, ``ws`` = wino4_workspace(..., m=6)); bf16x3=True: the three bf16 pieces of a 1x1 kernel (FRTM_WLAYOUT_BF16X3,
    Cin % 16 == 0; conv2d with ``w_layout=5``); bf16x1=True: the weights rounded to one bf16 plane (FRTM_WLAYOUT_BF16X1, Cin % 16 == 0; conv2d with
    ``w_layout=6``, ``tile`` 0 = automatic, 1 = 128x64, 2 = 64x64) -- or, for a 3x3 kernel, the bf16 image of the direct 3x3 form
    (FRTM_WLAYOUT_BF16X1_3X3, any Cin; conv2d with ``w_layout=7``, stride 1, pad 1, ``tile`` 0 = automatic, 1 = 64, 2 = 96 output channels); with
    ``stride=2`` the same image under FRTM_WLAYOUT_BF16X1_3X3_S2 (conv2d with ``w_layout=8``, stride 2, pad 1).
    Returns (wT, ktab, layout)."""
    w = w_oihw.detach().float().contiguous()
    Cout, Cin, k, _ = w.shape
    if bf16x1 and k == 3:
        layout = 8 if stride == 2 else 7
        wT = torch.zeros(bf16x1_3x3_elems(Cout, Cin), device=w.device)
        H.call('frtm_conv_pack_weights', H.ptr(w), Cout, Cin, k, layout, H.ptr(wT), None)
        return wT, None, layout
    if bf16x1:
        wT = torch.zeros(bf16x1_elems(Cout, Cin), device=w.device)
        H.call('frtm_conv_pack_weights', H.ptr(w), Cout, Cin, k, 6, H.ptr(wT), None)
        return wT, None, 6
    if bf16x3:
        wT = torch.zeros(bf16x3_elems(Cout, Cin), device=w.device)
        H.call('frtm_conv_pack_weights', H.ptr(w), Cout, Cin, k, 5, H.ptr(wT), None)
        return wT, None, 5
    layout = 4 if wino6 else 3 if wino4 else 2 if wino else (1 if (halo if halo is not None else k == 3) else 0)
    rows = 64 * padded_rows(Cin) if layout == 4 else 36 * padded_rows(Cin) if layout == 3 else max(padded_rows(Cin * k * k), (Cin + 7) // 8 * 72) if layout != 2 else (Cin + 7) // 8 * 128
    wT = torch.zeros(rows, padded_cols(Cout), device=w.device)
    ktab = torch.empty(Cin * k * k * 3, device=w.device, dtype=torch.int32) if (k > 1 and layout == 0) else None
    H.call('frtm_conv_pack_weights', H.ptr(w), Cout, Cin, k, layout, H.ptr(wT), H.ptr(ktab))
    return wT, ktab, layout


def wino4_workspace(B, Cin, Cout, Hh, Ww, device, m=4):
    """Scratch of a FRTM_WLAYOUT_WINO4 (m = 4) / WINO6 (m = 6) launch: the transformed input and product tensors
    (FRTM_CONV_WINO4_WS_ELEMS / FRTM_CONV_WINO6_WS_ELEMS)."""
    tiles = (B * ((Hh + m - 1) // m) * ((Ww + m - 1) // m) + 63) // 64 * 64
    return torch.empty((m + 2) ** 2 * (Cin + Cout) * tiles, device=device)


def act_to_bf16(x):
    """(B,C,H,W) float tensor -> the bf16 activation layout FRTM_ACT_BF16 of include/frtm_hip.h as a flat bfloat16 tensor: element (img, c, p) at
    index ((img * C/8 + c/8) * H*W + p) * 8 + c%8, rounded to nearest even.  Plain torch ops, for tests and tools: the trunk converts nowhere."""
    B, C, Hh, Ww = x.shape
    if C % 8:
        raise ValueError('act_to_bf16: the bf16 activation layout needs C %% 8 == 0 (got %d)' % C)
    return x.to(torch.bfloat16).reshape(B, C // 8, 8, Hh * Ww).permute(0, 1, 3, 2).contiguous().reshape(-1)


def act_from_bf16(buf, shape):
    """The inverse of act_to_bf16: a flat bfloat16 buffer in the FRTM_ACT_BF16 layout of a ``shape`` = (B,C,H,W) tensor -> float32 NCHW (exact)."""
    B, C, Hh, Ww = shape
    if C % 8 or buf.dtype != torch.bfloat16 or buf.numel() != B * C * Hh * Ww:
        raise ValueError('act_from_bf16: needs C %% 8 == 0 and a bfloat16 buffer of B*C*H*W elements')
    return buf.reshape(B, C // 8, Hh * Ww, 8).permute(0, 1, 3, 2).reshape(B, C, Hh, Ww).float().contiguous()


def conv2d(x, wT, Cout, ksize=1, stride=1, pad=0, ktab=None, scale=None, shift=None, residual=None, relu=False,
           out=None, out_transposed=False, splitk=0, tile=0, shape=None, w_pitch=0, w_layout=0, ws=None, in_fmt=0, res_fmt=0, out_fmt=0):
    """fp32 MFMA implicit-GEMM convolution.  x: (B,Cin,H,W) dense (or any dense buffer when ``shape``
    = (B,Cin,H,W) is given explicitly); wT: packed weights from pack_weights(), or a plain [K, w_pitch]
    matrix when w_pitch > 0.  Returns (B,Cout,Ho,Wo) (or (B,Ho*Wo,Cout)
    when out_transposed).
    ``in_fmt`` / ``res_fmt`` / ``out_fmt`` = 1 (FRTM_ACT_BF16; bf16x1 layouts 6, 7, 8 only, frtm_conv2d_act): x / residual is a flat bfloat16 buffer
    from act_to_bf16 (``shape`` is then required) / the result is one (read it with act_from_bf16)."""
    B, Cin, Hin, Win = shape if shape is not None else x.shape
    Ho = (Hin + 2 * pad - ksize) // stride + 1
    Wo = (Win + 2 * pad - ksize) // stride + 1
    if in_fmt or res_fmt or out_fmt:
        for name, t, fmt in (('x', x, in_fmt), ('residual', residual, res_fmt), ('out', out, out_fmt)):
            if t is not None and t.dtype != (torch.bfloat16 if fmt else torch.float32):
                raise TypeError('conv2d: %s must be %s under format %d' % (name, 'bfloat16' if fmt else 'float32', fmt))
        if out is None:
            out = torch.empty(B * Cout * Ho * Wo, device=x.device, dtype=torch.bfloat16) if out_fmt else torch.empty((B, Cout, Ho, Wo), device=x.device)
        d = H.ConvDesc(B, Cin, Hin, Win, Cout, ksize, stride, pad, int(relu), int(out_transposed), int(splitk), int(tile), int(w_layout), 0, int(w_pitch))
        H.call('frtm_conv2d_act', ctypes.byref(d), H.ptr(x), H.ptr(wT), H.ptr(ktab), H.ptr(scale), H.ptr(shift), H.ptr(residual), H.ptr(out), None,
               int(in_fmt), int(res_fmt), int(out_fmt))
        return out
    if out is None:
        out = torch.empty((B, Ho * Wo, Cout) if out_transposed else (B, Cout, Ho, Wo), device=x.device, dtype=torch.float32)
    if w_pitch > 0 and (w_pitch % 4 or wT.data_ptr() % 16):
        # frtm_conv2d reads a plain [K][w_pitch] matrix in 16-byte pieces: a pitch that is no multiple of 4 (a target model whose c is
        # none: the matrices of DiscriminatorLoss are dense (., c)) or a misaligned start goes through a zero-padded copy
        K, pitch = Cin * ksize * ksize, (int(w_pitch) + 3) // 4 * 4
        staged = torch.zeros(K, pitch, device=x.device, dtype=torch.float32)
        staged[:, :w_pitch].copy_(wT.reshape(-1)[:K * w_pitch].view(K, w_pitch))
        wT, w_pitch = staged, pitch
    out_elems = Cout * B * Ho * Wo
    # split-K only happens for small outputs (< ~800 workgroups); the library clamps the factor to the capacity given here
    # `ws`: the caller's own split-K scratch (hipGraphs that may replay concurrently must not share the per-stream one)
    if ws is None and splitk != 1:
        ws = workspace(x.device, min(32 * out_elems, max(2 * out_elems, 1 << 24)))
    d = H.ConvDesc(B, Cin, Hin, Win, Cout, ksize, stride, pad, int(relu), int(out_transposed), int(splitk), int(tile), int(w_layout),
                   0 if ws is None else min(ws.numel(), 0x7fffffff), int(w_pitch))
    H.call('frtm_conv2d', ctypes.byref(d), H.ptr(x), H.ptr(wT), H.ptr(ktab), H.ptr(scale), H.ptr(shift),
           H.ptr(residual), H.ptr(out), H.ptr(ws))
    return out


def filter_scores(X, f, out=None, accumulate=False, n=None, interleave=None):
    """(N,C,h,w) x (1,C,3,3) -> (N,1,h,w).
    ``interleave`` = (batch, k, groups): write map i to batch[i * groups + k] instead (batch: (N * groups, 1, h, w) dense) -- the
    frame-major (frame, object) score batch of a tracking window, filled object by object without a torch.stack afterwards."""
    N = X.shape[0] if n is None else n
    C, h, w = X.shape[1:]
    if interleave is not None:
        batch, k, groups = interleave
        assert batch.is_contiguous() and batch.shape[0] == N * groups and tuple(batch.shape[-2:]) == (h, w)
        H.call('frtm_filter_scores_pitched', H.ptr(X), H.ptr(f), N, C, h, w, batch.data_ptr() + 4 * k * h * w, groups * h * w, int(accumulate))
        return batch
    if out is None:
        out = torch.empty(N, 1, h, w, device=X.device)
    H.call('frtm_filter_scores', H.ptr(X), H.ptr(f), N, C, h, w, H.ptr(out), int(accumulate))
    return out


def pointer_table(tensors, device):
    """Device int64 table of the tensors' addresses (the w1T / w2 tables of target_apply_grouped), uploaded through pinned memory.
    The caller keeps the tensors alive and rebuilds the table when one of them moves."""
    return H.upload(torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64), device)


def target_apply_grouped(feats, frame_of_pair, w1T_table, w2_table, c, cft=None, scores=None):
    """Grouped target-model scoring (frtm_target_apply_grouped): for G (frame, target) pairs what G calls of
    Discriminator.apply_window on one frame each compute, in two launches.
    feats (F,Cin,h,w), frames dense inside but any pitch between them (a slice of a larger batch); frame_of_pair device int32 (G);
    w1T_table / w2_table device int64 (G) addresses of the [Cin][c] projections / (1,c,3,3) filters (pointer_table).
    Returns (cft (G,c,h,w), scores (G,1,h,w)); both may be given (dense, reused workspaces).  Raises on a shape the kernels refuse."""
    if feats.dim() != 4 or feats.dtype != torch.float32 or not feats.is_cuda:
        raise ValueError('target_apply_grouped: feats must be a (F,Cin,h,w) float32 tensor on the GPU (no CPU fallback)')
    F_, Cin, h, w = feats.shape
    if not feats[0].is_contiguous() or (F_ > 1 and feats.stride(0) < Cin * h * w):
        raise ValueError('target_apply_grouped: every frame of feats must be dense')
    G = frame_of_pair.numel()
    for name, t, dt in (('frame_of_pair', frame_of_pair, torch.int32), ('w1T_table', w1T_table, torch.int64), ('w2_table', w2_table, torch.int64)):
        if t.dtype != dt or t.device != feats.device or not t.is_contiguous() or t.numel() != G:
            raise ValueError('target_apply_grouped: %s must be a dense %s tensor of %d entries on %s' % (name, dt, G, feats.device))
    if cft is None:
        cft = torch.empty(G, c, h, w, device=feats.device)
    if scores is None:
        scores = torch.empty(G, 1, h, w, device=feats.device)
    if cft.numel() != G * c * h * w or scores.numel() != G * h * w or cft.dtype != torch.float32 or scores.dtype != torch.float32:
        raise ValueError('target_apply_grouped: cft must hold (G,c,h,w) and scores (G,1,h,w) float32')
    pitch = feats.stride(0) if F_ > 1 else Cin * h * w
    H.call('frtm_target_apply_grouped', H.ptr(feats[0]), pitch, F_, H.ptr(frame_of_pair), H.ptr(w1T_table), H.ptr(w2_table),
           G, Cin, int(c), h, w, H.ptr(cft), H.ptr(scores))
    return cft, scores


def transpose2d(x2d, out=None):
    rows, cols = x2d.shape
    if out is None:
        out = torch.empty(cols, rows, device=x2d.device)
    H.call('frtm_transpose2d', H.ptr(x2d), rows, cols, H.ptr(out))
    return out


def pixel_weights(y, tf):
    """Discriminator.compute_pixel_weights (hinge).  y (N,1,H,W) uint8/float in {0,1}."""
    y = y.contiguous()
    if y.dtype != torch.uint8:
        y = y.float()
    N, _, Hh, Ww = y.shape
    out = torch.empty(N, 1, Hh, Ww, device=y.device)
    scratch = torch.empty(N * 32, device=y.device)
    H.call('frtm_pixel_weights', H.ptr(y), int(y.dtype == torch.uint8), N, Hh, Ww, float(tf), H.ptr(out), H.ptr(scratch))
    return out


def merge_masks_(masks):
    """Tracker.track merge, in place on (n_obj+1,H,W), or on a window of frames (W,n_obj+1,H,W) in one launch."""
    if masks.dim() == 4:
        Wn, K, Hh, Ww = masks.shape
        H.call('frtm_merge_masks_frames', H.ptr(masks), Wn, K, Hh * Ww)
        return masks
    K, Hh, Ww = masks.shape
    H.call('frtm_merge_masks', H.ptr(masks), K, Hh * Ww)
    return masks


def count_above(masks, thr=0.5):
    """Per-plane pixel count above thr -> int32 (n) device tensor (no sync)."""
    m = masks.reshape(masks.shape[0], -1)
    cnt = torch.empty(m.shape[0], dtype=torch.int32, device=masks.device)
    H.call('frtm_count_above', H.ptr(m), m.shape[0], m.shape[1], float(thr), H.ptr(cnt))
    return cnt


def track_merge(logits, frames, n_obj, masks, labels=None, lut=None, single_object=False, counts=None, thr=0.5):
    """The tail of Tracker.track for a window in one pass (frtm_track_merge): refiner logits (frames * n_obj, 1, H, W), frame-major ->
    sigmoid -> merge -> ``masks`` (frames, n_obj + 1, H, W); optional ``labels`` (frames, 1, H, W) uint8 through ``lut`` (n_obj + 1
    device bytes) and ``counts`` (frames, n_obj + 1) int32 = pixels above ``thr`` per plane."""
    Hh, Ww = masks.shape[-2:]
    assert logits.is_contiguous() and masks.is_contiguous() and logits.shape[0] == frames * n_obj and masks.numel() == frames * (n_obj + 1) * Hh * Ww
    assert labels is None or (labels.is_contiguous() and labels.dtype == torch.uint8 and lut is not None and lut.dtype == torch.uint8)
    assert counts is None or (counts.is_contiguous() and counts.dtype == torch.int32 and counts.numel() == frames * (n_obj + 1))
    H.call('frtm_track_merge', H.ptr(logits), frames, n_obj, Hh * Ww, H.ptr(masks), None if labels is None else labels.data_ptr(),
           None if lut is None else lut.data_ptr(), int(bool(single_object)), None if counts is None else counts.data_ptr(), float(thr))
    return masks


# ----------------------------------------------------------------------------------------------------------------------
# Refiner glue (csrc/refiner_ops.hip; model/seg_network.py, model/refiner_train.py)
#
# One wrapper per entry point.  Every integer the C side takes is derived from the tensor shapes here, and what it cannot see (ranks,
# matching batch and channel counts, groups, dtype) is checked first and raises ValueError / TypeError: the library takes pointers, so a
# transposed h, w pair there is an out-of-bounds access, not an error message.  Weights arrive in the kernel's layout as tensors the caller
# holds; nothing but the result is allocated and nothing synchronises (safe under graph capture).  A single-frame window is bound by the
# host, so each check is one condition on the way through and the explanation (_refuse) is worked out only once it has failed.
# ----------------------------------------------------------------------------------------------------------------------
WINO_MIN_BLOCKS = 512        # FRTM_WINO_MIN_BLOCKS of include/frtm_hip.h


def wino_launch(n, h, w, cout):
    """The Winograd launch rule of the refiner's 3x3 convs (the trunk's: csrc/backbone.hip): F(2x2,3x3) when the launch has at least
    FRTM_WINO_MIN_BLOCKS 8x8 output blocks x 32-channel tiles, below that the halo layout with split-K."""
    return n * ((h + 7) // 8) * ((w + 7) // 8) * ((cout + 31) // 32) >= WINO_MIN_BLOCKS


def bf16x1_3x3_launch(n, h, w, cin, cout, min_blocks=None):
    """The ONE rule by which a bf16x1 refiner (SegNetwork.precision = 'bf16x1') routes a 3x3 conv to FRTM_WLAYOUT_BF16X1_3X3.
    ``min_blocks`` None: the measured rule (profiles/bf16x1_refiner_time.txt) -- BF16X1_3X3_ROUTES: a (cin, cout) pair is routed from the block
    count (wino_launch's count) of its smallest measured launch from which every measured launch's bf16 median beat the fp32 median by more than
    the fp32 arm's spread; only launches that wino_launch accepts were measured, so nothing below WINO_MIN_BLOCKS is routed.  A number: every
    3x3 conv whose launch has at least that many blocks (0 routes everything -- tests on small maps)."""
    blocks = n * ((h + 7) // 8) * ((w + 7) // 8) * ((cout + 31) // 32)
    if min_blocks is not None:
        return blocks >= min_blocks
    return blocks >= max(WINO_MIN_BLOCKS, BF16X1_3X3_ROUTES.get((cin, cout), 1 << 62))


# (cin, cout) -> fewest blocks per launch from which the measurement routes the refiner's 3x3 convs (see bf16x1_3x3_launch)
# (32, 64): the input gradient of the head's conv1 in a bf16x1 training pass (profiles/bf16x1_refiner_train_time.txt)
BF16X1_3X3_ROUTES = {(64, 64): 896, (65, 65): 5376, (65, 64): 12960, (64, 65): 9720, (64, 32): 25920, (32, 64): 51840}


def _refuse(fn, why, **tensors):
    """The slow path of a wrapper's argument check (the fast one is a single condition): TypeError for the first argument that is not a
    float32 tensor, else ValueError with what was expected and every shape."""
    for name, t in tensors.items():
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32):
            raise TypeError('%s: %s must be a float32 tensor, got %s' % (fn, name, t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
    raise ValueError('%s: %s; got %s' % (fn, why, ', '.join('%s %s' % (k, tuple(t.shape)) for k, t in tensors.items() if t is not None)))


_F32 = torch.float32


def plane_mean(x):
    """adaptive_avg_pool2d(x, 1) of x (N,C,H,W) -> (N,C)."""
    s = x.shape
    if len(s) != 4 or x.dtype is not _F32:
        _refuse('plane_mean', 'x must be (N,C,H,W)', x=x)
    out = torch.empty(s[0], s[1], device=x.device)
    H.call('frtm_plane_mean', H.ptr(x), s[0] * s[1], s[2] * s[3], H.ptr(out))
    return out


def pyrup2x(x):
    """PyrUpBicubic2d: (N,C,h,w) -> (N,C,2h,2w)."""
    s = x.shape
    if len(s) != 4 or x.dtype is not _F32:
        _refuse('pyrup2x', 'x must be (N,C,h,w)', x=x)
    n, c, h, w = s
    out = torch.empty(n, c, 2 * h, 2 * w, device=x.device)
    H.call('frtm_pyrup2x', H.ptr(x), n * c, h, w, H.ptr(out))
    return out


def bicubic_resize(x, size):
    """F.interpolate(x, size, mode='bicubic', align_corners=False) of x (N,C,h,w)."""
    s = x.shape
    Ho, Wo = int(size[-2]), int(size[-1])
    if len(s) != 4 or Ho < 1 or Wo < 1 or x.dtype is not _F32:
        _refuse('bicubic_resize', 'x must be (N,C,h,w) and the size %s positive' % ((Ho, Wo),), x=x)
    n, c, h, w = s
    out = torch.empty(n, c, Ho, Wo, device=x.device)
    H.call('frtm_bicubic_resize', H.ptr(x), n * c, h, w, H.ptr(out), Ho, Wo)
    return out


def tse_inject(base, bias, ws, scores, group):
    """relu(base[s // group] + bias + conv3x3(bilinear(scores[s]), ws)): base (F,C,H,W) the object-independent part of TSE.transform[0],
    bias (C), ws (C,9) its score-channel taps, scores (F * group,1,h,w) frame-major -> (F * group,C,H,W)."""
    bs, ss = base.shape, scores.shape
    group = int(group)
    if not (len(bs) == 4 == len(ss) and ss[1] == 1 and group > 0 and ss[0] == bs[0] * group and bias.numel() == bs[1] and ws.numel() == 9 * bs[1]
            and base.dtype is bias.dtype is ws.dtype is scores.dtype is _F32):
        _refuse('tse_inject', 'expected base (F,C,H,W), bias (C), ws (C,9) and scores (F * group,1,h,w) with group %d' % group,
                base=base, bias=bias, ws=ws, scores=scores)
    n, c = ss[0], bs[1]
    out = torch.empty(n, c, bs[2], bs[3], device=scores.device)
    H.call('frtm_tse_inject', H.ptr(base), H.ptr(bias), H.ptr(ws), H.ptr(scores), n, group, c, ss[2], ss[3], bs[2], bs[3], H.ptr(out))
    return out


def cab_gate(sp, dp, w1t, b1, w2t, b2, dp_group=0):
    """The CAB gate before its sigmoid: W2^T relu(W1^T cat(sp, dp) + b1) + b2.  sp (n,oc) pooled shallower and dp pooled deeper features,
    (n,oc) or, with dp_group > 0, one row per dp_group consecutive samples; w1t (2oc,oc), w2t (oc,oc): the 1x1 conv weights as [in][out]."""
    ss, ds = sp.shape, dp.shape
    g = int(dp_group)
    if not (len(ss) == 2 == len(ds) and g >= 0 and ds[0] * (g or 1) == ss[0] and ds[1] == ss[1] and ss[1] % 4 == 0
            and w1t.shape == (2 * ss[1], ss[1]) and w2t.numel() == ss[1] * ss[1] and b1.numel() == ss[1] == b2.numel()
            and sp.dtype is dp.dtype is w1t.dtype is b1.dtype is w2t.dtype is b2.dtype is _F32):
        _refuse('cab_gate', 'expected sp (n,oc), dp (n,oc) or (n / dp_group,oc) with dp_group %d, oc a multiple of 4, w1t (2oc,oc) and w2t (oc,oc) '
                'as [in][out], b1 and b2 (oc)' % g, sp=sp, dp=dp, w1t=w1t, b1=b1, w2t=w2t, b2=b2)
    n, oc = ss
    gate = torch.empty(n, oc, device=sp.device)
    H.call('frtm_cab_gate', H.ptr(sp), H.ptr(dp), g, H.ptr(w1t), H.ptr(b1), H.ptr(w2t), H.ptr(b2), n, oc, H.ptr(gate))
    return gate


def cab_combine(shallow, gate, deeper, deeper_group=0):
    """shallow * sigmoid(gate) + bilinear(deeper): shallow (n,C,H,W), gate (n,C), deeper (n,C,hd,wd) or a pooled (n,C) vector (hd = wd = 1);
    with deeper_group > 0, deeper holds one entry per deeper_group consecutive samples."""
    ss, ds = shallow.shape, deeper.shape
    g = int(deeper_group)
    if not (len(ss) == 4 and gate.shape == ss[:2] and len(ds) in (2, 4) and g >= 0 and ds[0] * (g or 1) == ss[0] and ds[1] == ss[1]
            and shallow.dtype is gate.dtype is deeper.dtype is _F32):
        _refuse('cab_combine', 'expected shallow (n,C,H,W), gate (n,C) and deeper (n,C,hd,wd) or (n,C), n / deeper_group entries with '
                'deeper_group %d' % g, shallow=shallow, gate=gate, deeper=deeper)
    hd, wd = (ds[2], ds[3]) if len(ds) == 4 else (1, 1)
    out = torch.empty_like(shallow)
    H.call('frtm_cab_combine', H.ptr(shallow), H.ptr(gate), H.ptr(deeper), ss[0], ss[1], hd, wd, g, ss[2], ss[3], H.ptr(out))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Frames with different object counts (csrc/ragged_group.hip): the indexed twins of tse_inject / cab_gate / cab_combine / track_merge.
# They take the table object, whose host-side counts every shape is checked against before anything touches a device.
# ----------------------------------------------------------------------------------------------------------------------
MAX_MERGE_OBJECTS = 15       # frtm_track_merge and frtm_track_merge_ragged: at most 15 objects per frame


class RaggedTable:
    """The sample-to-frame table of F frames that carry counts[f] objects each, samples frame-major: ``counts`` (host tuple), ``n`` = their
    sum, ``F``, ``frame_of`` (device int32 (n): the frame of every sample; also the frame_of_pair table of target_apply_grouped) and
    ``first`` (device int32 (F + 1): exclusive prefix sums; frame f owns samples first[f] .. first[f+1] - 1 and the mask planes
    first[f] + f .. first[f+1] + f of a packed merge buffer).  Every count is 1 .. 15 (the merge kernel's bound)."""

    def __init__(self, counts, device):
        counts = tuple(int(c) for c in counts)
        if not counts or any(c < 1 or c > MAX_MERGE_OBJECTS for c in counts):
            raise ValueError('RaggedTable: needs at least one frame and 1 .. %d objects on each, got %r' % (MAX_MERGE_OBJECTS, counts))
        self.counts, self.F, self.n = counts, len(counts), sum(counts)
        starts = [0]
        for c in counts:
            starts.append(starts[-1] + c)
        self.starts = tuple(starts)                                   # `first` on the host
        self.frame_of = H.upload(torch.tensor([f for f, c in enumerate(counts) for _ in range(c)], dtype=torch.int32), device)
        self.first = H.upload(torch.tensor(starts, dtype=torch.int32), device)

    def planes(self, f):
        """(start, stop) of frame f's n_f + 1 planes in a packed merge buffer."""
        return self.starts[f] + f, self.starts[f + 1] + f + 1


def tse_inject_indexed(base, bias, ws, scores, table):
    """tse_inject for frames with different object counts: relu(base[table.frame_of[s]] + bias + conv3x3(bilinear(scores[s]), ws)); base
    (table.F,C,H,W), scores (table.n,1,h,w) frame-major -> (table.n,C,H,W)."""
    bs, ss = base.shape, scores.shape
    if not (len(bs) == 4 == len(ss) and ss[1] == 1 and ss[0] == table.n and bs[0] == table.F and bias.numel() == bs[1] and ws.numel() == 9 * bs[1]
            and base.dtype is bias.dtype is ws.dtype is scores.dtype is _F32):
        _refuse('tse_inject_indexed', 'expected base (F,C,H,W), bias (C), ws (C,9) and scores (n,1,h,w) with F = %d frames of %r objects, '
                'n = %d' % (table.F, table.counts, table.n), base=base, bias=bias, ws=ws, scores=scores)
    n, c = ss[0], bs[1]
    out = torch.empty(n, c, bs[2], bs[3], device=scores.device)
    H.call('frtm_tse_inject_indexed', H.ptr(base), H.ptr(bias), H.ptr(ws), H.ptr(scores), n, H.ptr(table.frame_of), table.F, c, ss[2], ss[3],
           bs[2], bs[3], H.ptr(out))
    return out


def cab_gate_indexed(sp, dp, w1t, b1, w2t, b2, table):
    """cab_gate with the deeper pooled row of sample s = dp[table.frame_of[s]]: sp (table.n,oc), dp (table.F,oc)."""
    ss, ds = sp.shape, dp.shape
    if not (len(ss) == 2 == len(ds) and ss[0] == table.n and ds[0] == table.F and ds[1] == ss[1] and ss[1] % 4 == 0
            and w1t.shape == (2 * ss[1], ss[1]) and w2t.numel() == ss[1] * ss[1] and b1.numel() == ss[1] == b2.numel()
            and sp.dtype is dp.dtype is w1t.dtype is b1.dtype is w2t.dtype is b2.dtype is _F32):
        _refuse('cab_gate_indexed', 'expected sp (n,oc), dp (F,oc) with F = %d frames of %r objects, n = %d, oc a multiple of 4, w1t (2oc,oc) and '
                'w2t (oc,oc) as [in][out], b1 and b2 (oc)' % (table.F, table.counts, table.n), sp=sp, dp=dp, w1t=w1t, b1=b1, w2t=w2t, b2=b2)
    n, oc = ss
    gate = torch.empty(n, oc, device=sp.device)
    H.call('frtm_cab_gate_indexed', H.ptr(sp), H.ptr(dp), H.ptr(table.frame_of), table.F, H.ptr(w1t), H.ptr(b1), H.ptr(w2t), H.ptr(b2), n, oc,
           H.ptr(gate))
    return gate


def cab_combine_indexed(shallow, gate, deeper, table):
    """cab_combine with the deeper entry of sample s = deeper[table.frame_of[s]]: shallow (table.n,C,H,W), gate (table.n,C), deeper
    (table.F,C,hd,wd) or a pooled (table.F,C) vector (hd = wd = 1)."""
    ss, ds = shallow.shape, deeper.shape
    if not (len(ss) == 4 and gate.shape == ss[:2] and len(ds) in (2, 4) and ss[0] == table.n and ds[0] == table.F and ds[1] == ss[1]
            and shallow.dtype is gate.dtype is deeper.dtype is _F32):
        _refuse('cab_combine_indexed', 'expected shallow (n,C,H,W), gate (n,C) and deeper (F,C,hd,wd) or (F,C) with F = %d frames of %r objects, '
                'n = %d' % (table.F, table.counts, table.n), shallow=shallow, gate=gate, deeper=deeper)
    hd, wd = (ds[2], ds[3]) if len(ds) == 4 else (1, 1)
    out = torch.empty_like(shallow)
    H.call('frtm_cab_combine_indexed', H.ptr(shallow), H.ptr(gate), H.ptr(deeper), H.ptr(table.frame_of), table.F, ss[0], ss[1], hd, wd,
           ss[2], ss[3], H.ptr(out))
    return out


def track_merge_ragged(logits, table, masks, counts=None, thr=0.5):
    """track_merge for frames with different object counts (frtm_track_merge_ragged), no label decoding: refiner logits (table.n,1,H,W),
    frame-major -> sigmoid -> merge per frame -> ``masks`` (table.n + table.F, H, W): frame f's n_f + 1 planes are masks[table.planes(f)];
    optional ``counts`` (table.n + table.F) int32 = pixels above ``thr`` per plane, packed the same way."""
    ls, ms = logits.shape, masks.shape
    planes = table.n + table.F
    if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dtype is not torch.int32):
        raise TypeError('track_merge_ragged: counts must be an int32 tensor, got %s' % (counts.dtype if isinstance(counts, torch.Tensor) else type(counts).__name__))
    if not (len(ls) == 4 and ls[1] == 1 and ls[0] == table.n and len(ms) == 3 and ms[0] == planes and ms[1:] == ls[2:]
            and (counts is None or counts.numel() == planes) and logits.dtype is masks.dtype is _F32):
        _refuse('track_merge_ragged', 'expected logits (n,1,H,W) and masks (n + F,H,W) with F = %d frames of %r objects, n = %d, and %d counts'
                % (table.F, table.counts, table.n, planes), logits=logits, masks=masks)
    H.call('frtm_track_merge_ragged', H.ptr(logits), table.F, H.ptr(table.first), ls[2] * ls[3], H.ptr(masks),
           None if counts is None else H.ptr(counts), float(thr))
    return masks


def tap_mix(y, w2):
    """conv2's channel sum taken before the resampling: y (n,C,h,w), w2 (1,C,3,3) -> the nine tap maps (n,9,h,w)."""
    s = y.shape
    if not (len(s) == 4 and w2.numel() == 9 * s[1] and y.dtype is w2.dtype is _F32):
        _refuse('tap_mix', 'expected y (n,C,h,w) and w2 (1,C,3,3)', y=y, w2=w2)
    n, c, h, w = s
    out = torch.empty(n, 9, h, w, device=y.device)
    H.call('frtm_tap_mix', H.ptr(y), n, c, h * w, H.ptr(w2), H.ptr(out))
    return out


@functools.lru_cache(maxsize=None)
def _tail_fits(bicubic, h, w, Ho, Wo):
    return bool(H.lib().frtm_project_tail_fits(bicubic, h, w, Ho, Wo))


def project_tail_fits(h, w, size, bicubic=False):
    """Whether project_tail takes a (h,w) map -> ``size``: the library's own argument check (frtm_project_tail_fits; a pure function of five
    integers, remembered per argument set so that a window's head costs no call into the library)."""
    return _tail_fits(int(bool(bicubic)), int(h), int(w), int(size[-2]), int(size[-1]))


def project_tail(y, w3x3, bias, size, bicubic=False):
    """The fused tail of a head: conv2(resample(y)) + bias -> (n,1,Ho,Wo) with y (n,C,h,w), w3x3 (1,C,3,3), bias (1) or None; the resampling is
    up2 + bilinear to ``size`` (frtm_project_tail) or, ``bicubic``, a bicubic resize to it (frtm_project_tail_bicubic).  The resize must
    satisfy project_tail_fits."""
    s = y.shape
    Ho, Wo = int(size[-2]), int(size[-1])
    if not (len(s) == 4 and Ho > 0 and Wo > 0 and w3x3.numel() == 9 * s[1] and y.dtype is w3x3.dtype is _F32
            and (bias is None or (bias.numel() == 1 and bias.dtype is _F32))):
        _refuse('project_tail', 'expected y (n,C,h,w), w3x3 (1,C,3,3), bias (1) or None and a positive size, not %s' % ((Ho, Wo),),
                y=y, w3x3=w3x3, bias=bias)
    n, c, h, w = s
    out = torch.empty(n, 1, Ho, Wo, device=y.device)
    H.call('frtm_project_tail_bicubic' if bicubic else 'frtm_project_tail', H.ptr(y), n, c, h, w, H.ptr(w3x3), H.ptr(bias), Ho, Wo, H.ptr(out))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Refiner training (csrc/refiner_train.hip; model/refiner_train.py)
# ----------------------------------------------------------------------------------------------------------------------
def conv_wgrad(dy, x, k, weight=True, bias=True, bf16x1=False):
    """Gradients of a stride-1, pad-k//2 conv (k = 1 or 3) from its output gradient dy (B,Cout,H,W) and input x (B,Cin,H,W):
    (dW (Cout,Cin,k,k) or None, dbias (Cout) or None).  Deterministic: fixed-order sums, no atomics.  ``bf16x1`` (k = 3 only): the bf16x1
    form (frtm_conv_wgrad_bf16x1: both operands rounded to bf16 once, bf16 MFMAs, fp32 accumulation) -- NOT fp32-level arithmetic."""
    B, Cout, Hh, Ww = dy.shape
    Cin = x.shape[1]
    assert tuple(x.shape) == (B, Cin, Hh, Ww) and (weight or bias)
    if bf16x1 and k != 3:
        raise ValueError('conv_wgrad: the bf16x1 form is a 3x3 weight gradient (k = 3), got k = %d' % k)
    elems = H.lib().frtm_conv_wgrad_bf16x1_ws_elems(B, Cout, Cin, Hh, Ww) if bf16x1 else H.lib().frtm_conv_wgrad_ws_elems(B, Cout, Cin, k, Hh, Ww)
    # its own slab buffer: growing the shared conv workspace would change the split-K factor frtm_conv2d picks for later convs
    ws = torch.empty(elems, device=dy.device)
    dw = torch.empty(Cout, Cin, k, k, device=dy.device) if weight else None
    db = torch.empty(Cout, device=dy.device) if bias else None
    if bf16x1:
        H.call('frtm_conv_wgrad_bf16x1', H.ptr(dy), H.ptr(x), B, Cout, Cin, Hh, Ww, H.ptr(dw), H.ptr(db), H.ptr(ws), ws.numel())
    else:
        H.call('frtm_conv_wgrad', H.ptr(dy), H.ptr(x), B, Cout, Cin, k, Hh, Ww, H.ptr(dw), H.ptr(db), H.ptr(ws), ws.numel())
    return dw, db


def bf16x1_wgrad_launch(B, h, w, cin, cout, min_blocks=None):
    """The ONE rule by which a bf16x1 refiner training pass (SegNetwork.train_precision = 'bf16x1') routes a 3x3 weight gradient to
    frtm_conv_wgrad_bf16x1.  The block count is bf16x1_3x3_launch's, of the conv whose gradient it is.  ``min_blocks`` None: the measured rule
    (profiles/bf16x1_refiner_train_time.txt) -- BF16X1_WGRAD_ROUTES: a (cin, cout) pair is routed from the block count of its smallest measured
    launch from which every measured launch's bf16 median beat the fp32 median by more than the fp32 arm's spread; an unmeasured pair stays
    fp32.  A number: every 3x3 weight gradient whose conv has at least that many blocks (0 routes everything -- tests on small maps)."""
    blocks = B * ((h + 7) // 8) * ((w + 7) // 8) * ((cout + 31) // 32)
    if min_blocks is not None:
        return blocks >= min_blocks
    return blocks >= BF16X1_WGRAD_ROUTES.get((cin, cout), 1 << 62)


# (cin, cout) -> fewest blocks from which the measurement routes the refiner's 3x3 weight gradients (see bf16x1_wgrad_launch)
BF16X1_WGRAD_ROUTES = {(64, 32): 128, (64, 64): 896, (65, 64): 896, (65, 65): 384}


def bn_stats(x, running_mean, running_var, eps, factor, train):
    """Per-channel (mean, 1/sqrt(var + eps)) of x (N,C,H,W): batch statistics when ``train`` (the running ones updated in place with
    ``factor`` unless they are None or factor is 0), else the running statistics."""
    N, C, Hh, Ww = x.shape
    mean = torch.empty(C, device=x.device)
    invstd = torch.empty(C, device=x.device)
    part = torch.empty(2 * N * C, device=x.device, dtype=torch.float64) if train else None
    H.call('frtm_bn_stats', H.ptr(x), N, C, Hh * Ww, float(eps), float(factor), int(bool(train)), H.ptr(running_mean), H.ptr(running_var),
           H.ptr(mean), H.ptr(invstd), H.ptr(part))
    return mean, invstd


def bn_apply_relu(x, mean, invstd, gamma, beta):
    N, C, Hh, Ww = x.shape
    out = torch.empty_like(x)
    H.call('frtm_bn_apply_relu', H.ptr(x), H.ptr(mean), H.ptr(invstd), H.ptr(gamma), H.ptr(beta), N, C, Hh * Ww, H.ptr(out))
    return out


def bn_relu_backward(dy, out, x, mean, invstd, gamma, train, affine=True):
    """Backward of relu(batch_norm(x)) from the saved output: (dx, dgamma, dbeta); the last two None unless ``affine``."""
    N, C, Hh, Ww = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(C, device=x.device) if affine else None
    db = torch.empty(C, device=x.device) if affine else None
    part = torch.empty(3 * N * C, device=x.device, dtype=torch.float64)
    H.call('frtm_bn_relu_backward', H.ptr(dy), H.ptr(out), H.ptr(x), H.ptr(mean), H.ptr(invstd), H.ptr(gamma), N, C, Hh * Ww, int(bool(train)),
           H.ptr(dx), H.ptr(dg), H.ptr(db), H.ptr(part))
    return dx, dg, db


def relu_backward(dy, y, out=None):
    out = torch.empty_like(dy) if out is None else out
    H.call('frtm_relu_backward', H.ptr(dy), H.ptr(y), dy.numel(), H.ptr(out))
    return out


def pyrup2x_backward(dout):
    """Transpose of frtm_pyrup2x: (N,C,2h,2w) -> (N,C,h,w)."""
    N, C, H2, W2 = dout.shape
    h, w = H2 // 2, W2 // 2
    tmp = torch.empty(N * C * H2 * w, device=dout.device)
    din = torch.empty(N, C, h, w, device=dout.device)
    H.call('frtm_pyrup2x_backward', H.ptr(dout), N * C, h, w, H.ptr(din), H.ptr(tmp))
    return din


def bilinear_backward(dout, h, w):
    """Transpose of frtm_bilinear_resize (h,w) -> dout's size: (N,C,Ho,Wo) -> (N,C,h,w)."""
    N, C, Ho, Wo = dout.shape
    tmp = torch.empty(N * C * Ho * w, device=dout.device)
    din = torch.empty(N, C, h, w, device=dout.device)
    H.call('frtm_bilinear_backward', H.ptr(dout), N * C, h, w, Ho, Wo, H.ptr(din), H.ptr(tmp))
    return din


def bilinear_resize(x, size):
    N, C, h, w = x.shape
    out = torch.empty(N, C, int(size[0]), int(size[1]), device=x.device)
    H.call('frtm_bilinear_resize', H.ptr(x), N * C, h, w, H.ptr(out), int(size[0]), int(size[1]))
    return out


def add_plane_(x, v, scale):
    """x[n, c] += v[n, c] * scale for every pixel (in place)."""
    N, C, Hh, Ww = x.shape
    H.call('frtm_add_plane', H.ptr(x), H.ptr(v), float(scale), N * C, Hh * Ww)
    return x


def shift9(dl):
    """The input gradient of a 3x3 conv's nine taps: dl (n,1,H,W) -> (n,9,H,W), dl shifted by each tap, 0 outside."""
    s = dl.shape
    if not (len(s) == 4 and s[1] == 1 and dl.dtype is _F32):
        _refuse('shift9', 'dl must be (n,1,H,W)', dl=dl)
    out = torch.empty(s[0], 9, s[2], s[3], device=dl.device)
    H.call('frtm_shift9', H.ptr(dl), s[0], s[2], s[3], H.ptr(out))
    return out


def cab_backward_reduce(dout, s):
    """Per plane of dout and the CAB's shallower input s (N,C,H,W): (sum dout * s, sum dout), each (N,C)."""
    ds = dout.shape
    if not (len(ds) == 4 and s.shape == ds and dout.dtype is s.dtype is _F32):
        _refuse('cab_backward_reduce', 'dout and s must be (N,C,H,W), one shape', dout=dout, s=s)
    a = torch.empty(ds[0], ds[1], device=dout.device)
    b = torch.empty(ds[0], ds[1], device=dout.device)
    H.call('frtm_cab_backward_reduce', H.ptr(dout), H.ptr(s), ds[0] * ds[1], ds[2] * ds[3], H.ptr(a), H.ptr(b))
    return a, b


def cab_gate_backward(sp, dp, gate, a, badd, w1, b1, w2, grads=(True, True, True, True)):
    """Backward of cab_gate and the sigmoid from a = sum dout * s: sp, dp, gate, a (n,oc); badd (n,oc) or None is added to ddp; w1 (oc,2oc,1,1)
    and w2 (oc,oc,1,1) in the conv layout, b1 (oc).  -> (dW1, db1, dW2, db2, dsp, ddp), the first four shaped like the parameters and None
    where ``grads`` is false."""
    ss = sp.shape
    if not (len(ss) == 2 and dp.shape == ss and gate.shape == ss and a.shape == ss and (badd is None or (badd.shape == ss and badd.dtype is _F32))
            and w1.numel() == 2 * ss[1] * ss[1] and b1.numel() == ss[1] and w2.numel() == ss[1] * ss[1]
            and sp.dtype is dp.dtype is gate.dtype is a.dtype is w1.dtype is b1.dtype is w2.dtype is _F32):
        _refuse('cab_gate_backward', 'expected sp, dp, gate, a and badd (or None) of one shape (n,oc), w1 (oc,2oc,1,1), b1 (oc) and w2 (oc,oc,1,1)',
                sp=sp, dp=dp, gate=gate, a=a, badd=badd, w1=w1, b1=b1, w2=w2)
    n, oc = ss
    dsp = torch.empty(n, oc, device=sp.device)
    ddp = torch.empty(n, oc, device=sp.device)
    gw = [torch.empty_like(p) if g else None for p, g in zip((w1, b1, w2, b1), grads)]
    H.call('frtm_cab_gate_backward', H.ptr(sp), H.ptr(dp), H.ptr(gate), H.ptr(a), H.ptr(badd), H.ptr(w1), H.ptr(b1), H.ptr(w2), n, oc,
           *[H.ptr(g) for g in gw], H.ptr(dsp), H.ptr(ddp))
    return (*gw, dsp, ddp)


def cab_backward_shallow(dout, gate, dsp):
    """dout * sigmoid(gate) + dsp / (H * W): the gradient of the CAB's shallower input; dout (N,C,H,W), gate and dsp (N,C)."""
    ds = dout.shape
    if not (len(ds) == 4 and gate.shape == ds[:2] and dsp.shape == ds[:2] and dout.dtype is gate.dtype is dsp.dtype is _F32):
        _refuse('cab_backward_shallow', 'expected dout (N,C,H,W), gate and dsp (N,C)', dout=dout, gate=gate, dsp=dsp)
    out = torch.empty_like(dout)
    H.call('frtm_cab_backward_shallow', H.ptr(dout), H.ptr(gate), H.ptr(dsp), ds[0] * ds[1], ds[2] * ds[3], H.ptr(out))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# DAVIS J / F scoring (csrc/jf_eval.hip; lib/davis.py)
# ----------------------------------------------------------------------------------------------------------------------
JF_MAX_RADIUS = 64
JF_WS_BUDGET = 32 << 20        # bytes of boundary bit planes per call into the library; longer sequences go in frame chunks


def jf_counts(pred, truth, obj_ids, radius):
    """The integer counts behind J and F (frtm_jf_counts): pred / truth (T,H,W) uint8 or int32 label maps on the GPU, ``obj_ids`` K ints,
    ``radius`` of the matching disk in pixels (1 ... 64) -> (T,K,6) int32 device tensor = inter, union, n_fg, n_gt, fg_match, gt_match
    per (frame, object).  Enqueued on the current stream; no host synchronisation."""
    for name, t in (('pred', pred), ('truth', truth)):
        if not isinstance(t, torch.Tensor):
            raise TypeError('jf_counts: %s must be a tensor, got %s' % (name, type(t).__name__))
        if not t.is_cuda:
            raise RuntimeError('jf_counts: %s is on %s; the J / F kernels run on the GPU only (no CPU fallback; lib/davis.py has the '
                               'numpy definition)' % (name, t.device))
    if pred.device != truth.device:
        raise ValueError('jf_counts: pred on %s, truth on %s' % (pred.device, truth.device))
    if pred.dtype != truth.dtype or pred.dtype not in (torch.uint8, torch.int32):
        raise TypeError('jf_counts: label maps must both be uint8 or both int32, got %s and %s' % (pred.dtype, truth.dtype))
    if pred.dim() != 3 or pred.shape != truth.shape or pred.numel() == 0:
        raise ValueError('jf_counts: expected two (T,H,W) label maps of one non-empty shape, got %s and %s' % (tuple(pred.shape), tuple(truth.shape)))
    r = int(radius)
    if not 1 <= r <= JF_MAX_RADIUS:
        raise ValueError('jf_counts: disk radius %d outside 1 ... %d' % (r, JF_MAX_RADIUS))
    ids = [int(i) for i in obj_ids]
    T, Hh, Ww = pred.shape
    K = len(ids)
    counts = torch.empty(T, K, 6, dtype=torch.int32, device=pred.device)
    if K == 0:
        return counts
    pred, truth = pred.contiguous(), truth.contiguous()
    L = H.lib()
    ids_c = (ctypes.c_int * K)(*ids)
    per_frame = L.frtm_jf_workspace_bytes(1, Hh, Ww, K)
    step = max(1, min(JF_WS_BUDGET // per_frame, 65535 // (2 * K), T))
    ws = torch.empty(step * per_frame, dtype=torch.uint8, device=pred.device)
    for t0 in range(0, T, step):
        n = min(step, T - t0)
        H.call('frtm_jf_counts', H.ptr(pred[t0:t0 + n]), H.ptr(truth[t0:t0 + n]), pred.element_size(), n, Hh, Ww, ids_c, K, r,
               H.ptr(counts[t0:t0 + n]), H.ptr(ws), ws.numel())
    return counts


# ----------------------------------------------------------------------------------------------------------------------
# The ends of a training step (csrc/train_step.hip; model/train_loss.py, lib/fused_adam.py)
# ----------------------------------------------------------------------------------------------------------------------
def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def bce_logits(logits, target, grad=True):
    """The loss tail in one pass (frtm_bce_logits): logits (N,1,H,W) fp32, target of the same shape, uint8 {0,1} or fp32 in [0,1] ->
    (loss () fp32 = BCELoss(sigmoid(logits), target) as a function of real numbers, dlogits (N,1,H,W) or None unless ``grad``,
    inter (N) int32, union (N) int32: the counts behind mask_iou).  All on the device, deterministic, no host synchronisation."""
    for name, t in (('logits', logits), ('target', target)):
        if not isinstance(t, torch.Tensor):
            raise TypeError('bce_logits: %s must be a tensor, got %s' % (name, type(t).__name__))
        if not t.is_cuda:
            raise RuntimeError('bce_logits: %s is on %s; the loss kernel runs on the GPU only (no CPU fallback)' % (name, t.device))
    if logits.device != target.device:
        raise ValueError('bce_logits: logits on %s, target on %s' % (logits.device, target.device))
    if logits.dim() != 4 or logits.shape[1] != 1 or logits.numel() == 0:
        raise ValueError('bce_logits: expected (N,1,H,W) logits, got %s' % (tuple(logits.shape),))
    if tuple(target.shape) != tuple(logits.shape):
        raise ValueError('bce_logits: logits %s and target %s differ in size' % (tuple(logits.shape), tuple(target.shape)))
    if logits.dtype != torch.float32 or target.dtype not in (torch.float32, torch.uint8):
        raise TypeError('bce_logits: expected fp32 logits and uint8 / fp32 targets, got %s and %s' % (logits.dtype, target.dtype))
    N, _, Hh, Ww = logits.shape
    z, t = _aligned16(logits.detach().contiguous()), _aligned16(target.detach().contiguous())
    dev = z.device
    dz = torch.empty_like(z) if grad else None
    loss = torch.empty((), device=dev)
    counts = torch.empty(2, N, dtype=torch.int32, device=dev)
    ws = torch.empty(H.lib().frtm_bce_logits_workspace_bytes(N, Hh, Ww) // 8, dtype=torch.float64, device=dev)
    H.call('frtm_bce_logits', H.ptr(z), H.ptr(t), t.element_size(), N, Hh, Ww, H.ptr(dz), H.ptr(loss), H.ptr(counts[0]), H.ptr(counts[1]),
           H.ptr(ws), ws.numel() * 8)
    return loss, dz, counts[0], counts[1]


def adam_chunk_elems():
    return H.lib().frtm_adam_chunk_elems()


def adam_step(tensors, n_tensors, chunks, n_chunks, lr, bias_correction1, bias_correction2, beta1, beta2, eps, weight_decay, amsgrad):
    """One launch of frtm_adam_amsgrad over the device tables ``tensors`` (int64, 8 words per tensor) and ``chunks`` (int32 pairs);
    lib/fused_adam.py builds them."""
    assert tensors.is_cuda and tensors.dtype == torch.int64 and tensors.numel() == 8 * n_tensors
    assert chunks.is_cuda and chunks.dtype == torch.int32 and chunks.numel() == 2 * n_chunks
    H.call('frtm_adam_amsgrad', H.ptr(tensors), int(n_tensors), H.ptr(chunks), int(n_chunks), float(lr), float(bias_correction1),
           float(bias_correction2), float(beta1), float(beta2), float(eps), float(weight_decay), int(bool(amsgrad)))


def scale_by_(x, scale):
    """x *= scale in place, ``scale`` a one-element fp32 tensor on the device (frtm_scale_by): no read-back of the scalar."""
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and scale.dtype == torch.float32 and scale.numel() == 1
    H.call('frtm_scale_by', H.ptr(x), x.numel(), H.ptr(scale.contiguous()))
    return x


# ----------------------------------------------------------------------------------------------------------------------
# Batched resize of native-size training frames and label maps (csrc/frame_resize.hip; lib/training_datasets.py: DeviceFrameResizer)
# ----------------------------------------------------------------------------------------------------------------------
RESIZE_MODES = {'area': 0, 'cubic': 1}


def _resize_packed(entry, src, desc, planes, size):
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise RuntimeError('%s: the packed source is on %s; the resize kernels run on the GPU only (no CPU fallback)'
                           % (entry, getattr(src, 'device', type(src).__name__)))
    if src.dtype != torch.uint8 or src.dim() != 1:
        raise TypeError('%s: expected a flat uint8 buffer, got %s %s' % (entry, src.dtype, tuple(src.shape)))
    if not isinstance(desc, torch.Tensor) or desc.is_cuda or desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != 4 or desc.shape[0] < 1:
        raise TypeError('%s: the frame table is a CPU int64 tensor of shape (n, 4), n >= 1' % entry)
    desc = desc.contiguous()
    n = desc.shape[0]
    out = torch.empty(n, planes, int(size[0]), int(size[1]), dtype=torch.uint8, device=src.device)
    table = H.upload(desc, src.device)
    args = (H.ptr(src), src.numel(), desc.data_ptr(), H.ptr(table), n) + ((planes,) if entry == 'frtm_resize_frames_u8' else ())
    H.call(entry, *args, H.ptr(out), int(size[0]), int(size[1]))
    return out


def resize_frames_u8(src, desc, planes, size):
    """frtm_resize_frames_u8: ``src`` a flat uint8 device buffer of frames packed at any byte offsets, ``desc`` a CPU int64 (n,4) table
    of rows (offset, h, w, RESIZE_MODES[mode]), each frame ``planes`` planes of h x w bytes -> (n, planes, H, W) uint8 on the device.
    One launch, enqueued on the current stream."""
    return _resize_packed('frtm_resize_frames_u8', src, desc, int(planes), size)


def resize_labels_u8(src, desc, size):
    """frtm_resize_labels_u8: label maps packed like the frames (one plane each), ``desc`` rows (offset, h, w, obj_id) -> (n, 1, H, W)
    uint8 = (label == obj_id) at F.interpolate(mode='nearest')'s source indices.  One launch, enqueued on the current stream."""
    return _resize_packed('frtm_resize_labels_u8', src, desc, 1, size)


def resize_label_map_u8(src, desc, size):
    """frtm_resize_label_map_u8: label maps packed like the frames (one plane each), ``desc`` rows (offset, h, w, 0) -> (n, 1, H, W) uint8
    = the label at F.interpolate(mode='nearest')'s source indices, ids kept (resize_labels_u8 compares them with one id instead).  One
    launch, enqueued on the current stream."""
    return _resize_packed('frtm_resize_label_map_u8', src, desc, 1, size)


class ResizePlan:
    """A frame table of resize_frames_u8 / resize_labels_u8 / resize_label_map_u8 that is uploaded ONCE: those functions upload their table
    on every call (H.upload: an allocation and a copy), which a per-frame caller (Tracker.track under working_size, a StreamPool tick)
    should not pay.  ``desc`` as there: a CPU int64 (n, 4) table.  ``frames`` / ``labels`` / ``label_map`` are those three launches on the
    kept table; ``out``: the caller's (n, planes, H, W) uint8 buffer (else allocated)."""

    def __init__(self, desc, device):
        if not isinstance(desc, torch.Tensor) or desc.is_cuda or desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != 4 or desc.shape[0] < 1:
            raise TypeError('ResizePlan: the frame table is a CPU int64 tensor of shape (n, 4), n >= 1')
        self.desc = desc.contiguous().clone()                         # the host copy the library checks on every call: kept alive here
        self.n = self.desc.shape[0]
        self.table = H.upload(self.desc, device)

    def _run(self, entry, src, planes, size, out):
        if not isinstance(src, torch.Tensor) or not src.is_cuda:
            raise RuntimeError('%s: the packed source is on %s; the resize kernels run on the GPU only (no CPU fallback)'
                               % (entry, getattr(src, 'device', type(src).__name__)))
        if src.dtype != torch.uint8 or src.dim() != 1:
            raise TypeError('%s: expected a flat uint8 buffer, got %s %s' % (entry, src.dtype, tuple(src.shape)))
        shape = (self.n, planes, int(size[0]), int(size[1]))
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=src.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_cuda:
            raise TypeError('%s: out must be a uint8 device tensor of shape %r, got %s %s' % (entry, shape, out.dtype, tuple(out.shape)))
        args = (H.ptr(src), src.numel(), self.desc.data_ptr(), H.ptr(self.table), self.n) + ((planes,) if entry == 'frtm_resize_frames_u8' else ())
        H.call(entry, *args, H.ptr(out), shape[2], shape[3])
        return out

    def frames(self, src, planes, size, out=None):
        return self._run('frtm_resize_frames_u8', src, int(planes), size, out)

    def labels(self, src, size, out=None):
        return self._run('frtm_resize_labels_u8', src, 1, size, out)

    def label_map(self, src, size, out=None):
        return self._run('frtm_resize_label_map_u8', src, 1, size, out)


# ----------------------------------------------------------------------------------------------------------------------
# Decoder frames: NV12 surfaces (and planar RGB) to planar RGB at one size in one launch (csrc/frame_formats.hip)
# ----------------------------------------------------------------------------------------------------------------------
FRAME_FORMATS = {'rgb': 0, 'nv12_bt601': 1, 'nv12_bt601_full': 2, 'nv12_bt709': 3, 'nv12_bt709_full': 4}


def _frames_args(entry, src, desc):
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise RuntimeError('%s: the source buffer is on %s; the frame kernels run on the GPU only (no CPU fallback)'
                           % (entry, getattr(src, 'device', type(src).__name__)))
    if src.dtype != torch.uint8 or src.dim() != 1:
        raise TypeError('%s: expected a flat uint8 buffer, got %s %s' % (entry, src.dtype, tuple(src.shape)))
    if desc is not None and (not isinstance(desc, torch.Tensor) or desc.is_cuda or desc.dtype != torch.int64 or desc.dim() != 2
                             or desc.shape[1] != 8 or desc.shape[0] < 1):
        raise TypeError('%s: the frame table is a CPU int64 tensor of shape (n, 8), n >= 1' % entry)


def frames_to_rgb_u8(src, desc, size):
    """frtm_frames_to_rgb_u8: ``src`` a flat uint8 device buffer, ``desc`` a CPU int64 (n, 8) table of rows (offset, h, w,
    RESIZE_MODES[mode], FRAME_FORMATS[format], pitch, uv offset, 0) -> (n, 3, H, W) uint8 planar RGB on the device: each frame converted by
    the fixed-point formula of include/frtm_hip.h and put through resize_frames_u8's operator, bit for bit.  One launch, enqueued on the
    current stream; the table is uploaded per call (FramePlan keeps it)."""
    _frames_args('frtm_frames_to_rgb_u8', src, desc)
    desc = desc.contiguous()
    out = torch.empty(desc.shape[0], 3, int(size[0]), int(size[1]), dtype=torch.uint8, device=src.device)
    table = H.upload(desc, src.device)
    H.call('frtm_frames_to_rgb_u8', H.ptr(src), src.numel(), desc.data_ptr(), H.ptr(table), desc.shape[0], H.ptr(out), int(size[0]), int(size[1]))
    return out


class FramePlan:
    """A frame table of frames_to_rgb_u8 that is uploaded ONCE (ResizePlan's role for that launch).  ``desc``: a CPU int64 (n, 8) table;
    ``frames(src, size, out=None)``: the launch on the kept table, ``out`` the caller's (n, 3, H, W) uint8 buffer (else allocated)."""

    def __init__(self, desc, device):
        if not isinstance(desc, torch.Tensor) or desc.is_cuda or desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != 8 or desc.shape[0] < 1:
            raise TypeError('FramePlan: the frame table is a CPU int64 tensor of shape (n, 8), n >= 1')
        self.desc = desc.contiguous().clone()                         # the host copy the library checks on every call: kept alive here
        self.n = self.desc.shape[0]
        self.table = H.upload(self.desc, device)

    def frames(self, src, size, out=None):
        entry = 'frtm_frames_to_rgb_u8'
        _frames_args(entry, src, None)
        shape = (self.n, 3, int(size[0]), int(size[1]))
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=src.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_cuda:
            raise TypeError('%s: out must be a uint8 device tensor of shape %r, got %s %s'
                            % (entry, shape, getattr(out, 'dtype', type(out).__name__), tuple(getattr(out, 'shape', ()))))
        H.call(entry, H.ptr(src), src.numel(), self.desc.data_ptr(), H.ptr(self.table), self.n, H.ptr(out), shape[2], shape[3])
        return out


class DecoderFrame:
    """One NV12 surface as a hardware video decoder leaves it on the device, accepted wherever Tracker.initialize / track and
    StreamPool.initialize / step take a (3, H, W) uint8 frame.  ``data``: a flat uint8 CUDA tensor that STARTS at the Y plane (a view
    over the surface's memory: nothing is copied here); ``height`` x ``width``: the picture, 1 .. 16384 each, odd sizes allowed; ``pitch``:
    bytes from one row to the next in both planes (default 2 * ceil(width / 2): no padding); ``uv_offset``: byte offset of the interleaved
    U,V plane in ``data`` (default pitch * height; a coded height above the picture's is expressed by passing pitch * coded height);
    ``matrix`` 'bt601' or 'bt709', ``full_range``: which of the four conversions of include/frtm_hip.h applies.  Everything is
    checked here, on the host; no GPU work is done before the frame is used."""

    def __init__(self, data, height, width, pitch=None, uv_offset=None, matrix='bt709', full_range=False):
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1:
            raise TypeError('DecoderFrame: data is a flat uint8 tensor, got %s %s'
                            % (getattr(data, 'dtype', type(data).__name__), tuple(getattr(data, 'shape', ()))))
        self.height, self.width = int(height), int(width)
        self.pitch, self.uv_offset, self.nbytes_needed = self.layout(height, width, pitch, uv_offset)
        name = 'nv12_%s%s' % (matrix, '_full' if full_range else '')
        if matrix not in ('bt601', 'bt709') or name not in FRAME_FORMATS:
            raise ValueError("DecoderFrame: matrix is 'bt601' or 'bt709', got %r" % (matrix,))
        self.matrix, self.full_range = matrix, bool(full_range)
        self.format = FRAME_FORMATS[name]
        if data.numel() < self.nbytes_needed:
            raise ValueError('DecoderFrame: data holds %d bytes, the surface needs %d' % (data.numel(), self.nbytes_needed))
        if not data.is_cuda:
            raise RuntimeError('DecoderFrame: data is on %s; a decoder surface lives on the GPU (no CPU fallback)' % data.device)
        if not data.is_contiguous():
            raise TypeError('DecoderFrame: data must be contiguous')
        self.data = data
        self.shape = torch.Size((3, self.height, self.width))
        self.dtype = torch.uint8
        self.device = data.device

    @staticmethod
    def layout(height, width, pitch=None, uv_offset=None):
        """(pitch, uv_offset, nbytes_needed) of a surface with the defaults filled in; ValueError for a layout no surface has."""
        height, width = int(height), int(width)
        if not (1 <= height <= MAX_NATIVE_DIM and 1 <= width <= MAX_NATIVE_DIM):
            raise ValueError('DecoderFrame: picture size %d x %d (1 .. %d)' % (height, width, MAX_NATIVE_DIM))
        chroma_row = 2 * ((width + 1) // 2)
        pitch = chroma_row if pitch is None else int(pitch)
        if pitch < chroma_row:
            raise ValueError('DecoderFrame: pitch %d is below the %d bytes of a chroma row' % (pitch, chroma_row))
        uv_offset = pitch * height if uv_offset is None else int(uv_offset)
        if uv_offset < pitch * height:
            raise ValueError('DecoderFrame: uv_offset %d lies inside the Y plane (%d rows of pitch %d)' % (uv_offset, height, pitch))
        return pitch, uv_offset, uv_offset + pitch * ((height + 1) // 2)

    def row(self, offset=0, mode='area'):
        """This frame's row of a frames_to_rgb_u8 table, its Y plane at byte ``offset`` of the source buffer."""
        return [int(offset), self.height, self.width, RESIZE_MODES[mode], self.format, self.pitch, int(offset) + self.uv_offset, 0]

    def plan_key(self):
        """What a cached FramePlan of this frame depends on."""
        return (self.height, self.width, self.pitch, self.uv_offset, self.format)


# ----------------------------------------------------------------------------------------------------------------------
# The way back from a working size (csrc/native_size.hip; Tracker(working_size=...), StreamPool(working_size=...))
# ----------------------------------------------------------------------------------------------------------------------
MAX_NATIVE_DIM = 16384        # frtm_masks_to_native and the resize kernels: 1 .. 16384 pixels per axis


class NativeTable:
    """The frame table of masks_to_native, built once per (sizes, plane counts) and kept, like RaggedTable: ``rows`` a CPU int64 (n, 7)
    tensor of (offset of the frame's first plane in the mask buffer, K planes, native H, native W, offset of its label map in the label
    buffer, offset of its K planes in the soft buffer or -1, offset of its K-byte LUT), offsets in elements of the buffer they index.
    Every K is 1 .. MAX_MERGE_OBJECTS + 1 and every native size 1 .. 16384 (ValueError otherwise, on the host); a row whose offsets leave
    the buffers of a call is skipped by the kernel.  ``label_bytes`` / ``soft_elems`` / ``lut_bytes``: the smallest buffers that hold
    every row's output."""

    def __init__(self, rows, device):
        rows = torch.as_tensor(rows, dtype=torch.int64)
        if rows.dim() != 2 or rows.shape[1] != 7 or rows.shape[0] < 1 or rows.shape[0] > 65535:
            raise ValueError('NativeTable: rows are (n, 7), 1 <= n <= 65535, got %r' % (tuple(rows.shape),))
        self.rows = rows.contiguous().clone()
        for i, (_, K, Hn, Wn, _, _, _) in enumerate(self.rows.tolist()):
            if not 1 <= K <= MAX_MERGE_OBJECTS + 1:
                raise ValueError('NativeTable: frame %d has %d planes (1 .. %d)' % (i, K, MAX_MERGE_OBJECTS + 1))
            if not (1 <= Hn <= MAX_NATIVE_DIM and 1 <= Wn <= MAX_NATIVE_DIM):
                raise ValueError('NativeTable: frame %d has native size %d x %d (1 .. %d)' % (i, Hn, Wn, MAX_NATIVE_DIM))
        r = self.rows
        self.n = r.shape[0]
        self.label_bytes = int((r[:, 4] + r[:, 2] * r[:, 3]).max())
        self.soft_elems = int(torch.where(r[:, 5] >= 0, r[:, 5] + r[:, 1] * r[:, 2] * r[:, 3], torch.zeros_like(r[:, 5])).max())
        self.lut_bytes = int((r[:, 6] + r[:, 1]).max())
        self.dev = H.upload(self.rows, device)

    @classmethod
    def packed(cls, size, frames, device, soft=True, shared_lut=False):
        """The table of ``frames`` = (K, H, W) per frame whose planes lie one frame after the other in the mask buffer (a (F, K, h, w)
        stack, or the packed buffer of track_merge_ragged) at the working ``size``, with label maps, soft planes (``soft``) and LUTs
        packed in frame order as well; ``shared_lut``: every frame reads the LUT at offset 0 (frames of one sequence)."""
        h, w = int(size[0]), int(size[1])
        rows, mo, lo, so, to = [], 0, 0, 0, 0
        for K, Hn, Wn in frames:
            K, Hn, Wn = int(K), int(Hn), int(Wn)
            rows.append((mo, K, Hn, Wn, lo, so if soft else -1, 0 if shared_lut else to))
            mo, lo, so, to = mo + K * h * w, lo + Hn * Wn, so + K * Hn * Wn, to + K
        return cls(rows, device)

    def labels_of(self, labels, i):
        """Frame i's (H, W) label map in the flat label buffer of a call."""
        o, Hn, Wn = int(self.rows[i, 4]), int(self.rows[i, 2]), int(self.rows[i, 3])
        return labels[o:o + Hn * Wn].view(Hn, Wn)

    def soft_of(self, soft, i):
        """Frame i's (K, H, W) planes in the flat soft buffer of a call."""
        o, K, Hn, Wn = int(self.rows[i, 5]), int(self.rows[i, 1]), int(self.rows[i, 2]), int(self.rows[i, 3])
        return soft[o:o + K * Hn * Wn].view(K, Hn, Wn)


def masks_to_native(masks, table, labels, luts, soft=None, size=None):
    """frtm_masks_to_native: ``masks`` merged masks (..., h, w) float32 at the working size -- or, with ``size`` = (h, w) given, a buffer
    of any shape that holds the planes at the table's offsets --, read as one flat buffer through ``table``
    (NativeTable) -> ``labels`` (flat uint8 device buffer: every frame's native-size label map through its K bytes of ``luts``, flat
    uint8) and, for the rows that ask for them, the K native-size planes in ``soft`` (flat float32).  Per pixel: the bilinear sample of
    every plane (F.interpolate(mode='bilinear', align_corners=False); the plane itself on equal sizes), label = lut[arg-max] where the
    arg-max is an object above 0.5, else lut[0].  One launch for all frames, enqueued on the current stream.  -> (labels, soft)."""
    if not isinstance(masks, torch.Tensor) or masks.dtype is not _F32 or (soft is not None and (not isinstance(soft, torch.Tensor) or soft.dtype is not _F32)):
        _refuse('masks_to_native', 'masks and soft are float32', masks=masks, soft=soft)
    for name, t in (('labels', labels), ('luts', luts)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise TypeError('masks_to_native: %s must be a uint8 tensor, got %s' % (name, t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
    if masks.dim() < (2 if size is None else 1) or labels.dim() != 1 or luts.dim() != 1 or (soft is not None and soft.dim() != 1):
        _refuse('masks_to_native', 'expected masks (..., h, w) and flat labels, luts and soft buffers', masks=masks, soft=soft)
    if not isinstance(table, NativeTable):
        raise TypeError('masks_to_native: table must be an ops.NativeTable, got %s' % type(table).__name__)
    h, w = masks.shape[-2:] if size is None else (int(size[0]), int(size[1]))
    if not (1 <= h <= MAX_NATIVE_DIM and 1 <= w <= MAX_NATIVE_DIM):
        raise ValueError('masks_to_native: working size %d x %d (1 .. %d)' % (h, w, MAX_NATIVE_DIM))
    if soft is None and table.soft_elems > 0:
        raise ValueError('masks_to_native: the table asks for soft planes, but there is no soft buffer')
    if not (masks.is_cuda and labels.is_cuda and luts.is_cuda and (soft is None or soft.is_cuda)):
        raise RuntimeError('masks_to_native: tensors on %s; the kernel runs on the GPU only (no CPU fallback)' % (masks.device,))
    H.call('frtm_masks_to_native', H.ptr(masks), masks.numel(), int(h), int(w), table.rows.data_ptr(), H.ptr(table.dev), table.n,
           H.ptr(labels), labels.numel(), H.ptr(soft), 0 if soft is None else soft.numel(), H.ptr(luts), luts.numel())
    return labels, soft


# ----------------------------------------------------------------------------------------------------------------------
# The way out: tracked objects rendered onto RGB and NV12 frames in one launch (csrc/frame_render.hip)
# ----------------------------------------------------------------------------------------------------------------------
RENDER_FORMATS = {'rgb': 0, 'nv12': 1}              # FRTM_RENDER_RGB / FRTM_RENDER_NV12
RENDER_ANSWERS = {'labels': 0, 'masks': 1}          # FRTM_RENDER_LABELS / FRTM_RENDER_MASKS
RENDER_ROW_WORDS = 20                               # FRTM_RENDER_ROW_WORDS
# FRAME_FORMATS id of an NV12 format -> (y0, yr, yg, yb, ur, ug, ub, vr, vg, vb): the forward table of include/frtm_hip.h
RENDER_YUV = {
    1: (16, 16829, 33039, 6416, -9714, -19071, 28784, 28784, -24103, -4681),
    2: (0, 19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329),
    3: (16, 11966, 40254, 4064, -6596, -22189, 28784, 28784, -26145, -2639),
    4: (0, 13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005),
}


def rgb_to_yuv_u8(rgb, fmt):
    """(..., 3) integer RGB in 0..255 (a CPU tensor) -> (..., 3) uint8 (Y, U, V) by the forward fixed-point formula of include/frtm_hip.h
    for FRAME_FORMATS id ``fmt`` (1 .. 4): Y = clamp(y0 + ((yr R + yg G + yb B + 32768) >> 16)), U and V around 128 likewise."""
    y0, yr, yg, yb, ur, ug, ub, vr, vg, vb = RENDER_YUV[int(fmt)]
    c = rgb.to(torch.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    yuv = torch.stack([y0 + ((yr * r + yg * g + yb * b + 32768) >> 16), 128 + ((ur * r + ug * g + ub * b + 32768) >> 16),
                       128 + ((vr * r + vg * g + vb * b + 32768) >> 16)], dim=-1)
    return yuv.clamp_(0, 255).to(torch.uint8)


def _byte(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise TypeError('RenderStyle: %s is an integer 0 .. 255, got %r' % (name, v))
    v = int(v)
    if not 0 <= v <= 255:
        raise ValueError('RenderStyle: %s is 0 .. 255, got %d' % (name, v))
    return v


class RenderStyle:
    """How render_frames draws the objects: per object id a colour and an opacity.  ``palette``: (256, 3) uint8 RGB, numpy or torch
    (default: lib.image.davis_palette); ``alpha``: one 0 .. 255 opacity for all ids or a vector of 256; ``background``: None -- id 0 is left
    untouched (a_0 = 0 whatever ``alpha`` says) -- or (r, g, b, a): dim or replace the background; ``edge_alpha``: None, or the 0 .. 255
    opacity of an object's boundary pixels (hard rule only); ``soft``: blend by the winning mask's value instead of its label (mask stacks
    only).  ``table``: the (256, 4) uint8 CPU rows (r, g, b, a); the device tables -- in R,G,B, or in Y,U,V of one matrix and range -- are
    made once per (device, format) and kept."""

    def __init__(self, palette=None, alpha=128, background=None, edge_alpha=None, soft=False):
        if palette is None:
            from .lib.image import davis_palette as palette
        if not isinstance(palette, torch.Tensor):
            import numpy as np
            if not isinstance(palette, np.ndarray):
                raise TypeError('RenderStyle: palette is a (256, 3) uint8 array or tensor, got %s' % type(palette).__name__)
            palette = torch.from_numpy(np.ascontiguousarray(palette))
        if palette.dtype != torch.uint8:
            raise TypeError('RenderStyle: palette is uint8, got %s' % palette.dtype)
        if tuple(palette.shape) != (256, 3):
            raise ValueError('RenderStyle: palette is (256, 3), got %r' % (tuple(palette.shape),))
        table = torch.empty(256, 4, dtype=torch.uint8)
        table[:, :3] = palette.cpu()
        if isinstance(alpha, numbers.Integral) and not isinstance(alpha, bool):
            table[:, 3] = _byte('alpha', alpha)
        else:
            if isinstance(alpha, (bool, float, str)) or alpha is None:
                raise TypeError('RenderStyle: alpha is an integer 0 .. 255 or 256 of them, got %r' % (alpha,))
            a = torch.as_tensor(alpha)
            if a.dtype.is_floating_point or a.dtype == torch.bool or a.dtype.is_complex:
                raise TypeError('RenderStyle: alpha holds integers, got %s' % a.dtype)
            if tuple(a.shape) != (256,):
                raise ValueError('RenderStyle: an alpha vector has 256 entries, got %r' % (tuple(a.shape),))
            a = a.cpu().to(torch.int64)
            if int(a.min()) < 0 or int(a.max()) > 255:
                raise ValueError('RenderStyle: alpha is 0 .. 255')
            table[:, 3] = a.to(torch.uint8)
        if background is None:
            table[0, 3] = 0
        else:
            if isinstance(background, (str, bytes)) or not hasattr(background, '__len__'):
                raise TypeError('RenderStyle: background is None or (r, g, b, a), got %r' % (background,))
            if len(background) != 4:
                raise ValueError('RenderStyle: background is (r, g, b, a), got %d values' % len(background))
            table[0] = torch.tensor([_byte('background', v) for v in background], dtype=torch.uint8)
        self.edge_alpha = None if edge_alpha is None else _byte('edge_alpha', edge_alpha)
        if not isinstance(soft, bool):
            raise TypeError('RenderStyle: soft is a bool, got %r' % (soft,))
        if soft and self.edge_alpha is not None:
            raise ValueError('RenderStyle: edge_alpha belongs to the hard rule; soft has no edges')
        self.soft = soft
        self.table = table
        self._dev = {}

    def table_for(self, fmt):
        """The CPU (256, 4) uint8 table in the channels of FRAME_FORMATS id ``fmt``: (r, g, b, a) for 0, (y, u, v, a) for an NV12 format."""
        if int(fmt) == 0:
            return self.table
        t = self.table.clone()
        t[:, :3] = rgb_to_yuv_u8(self.table[:, :3], fmt)
        return t

    def device_table(self, device, fmt):
        key = (H.normalize_device(device), int(fmt))
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = H.upload(self.table_for(fmt).contiguous(), key[0])
        return t


_default_style = None
RENDER_TABLES_KEPT = 256                            # uploaded row tables render_frames keeps, least recently used first out
_render_tables = collections.OrderedDict()


def default_render_style():
    global _default_style
    if _default_style is None:
        _default_style = RenderStyle()
    return _default_style


def _render_surface(what, i, f, size=None, fmt=None):
    """(size, (FRAME_FORMATS id, tensor that holds the bytes, pitch, uv offset)) of frame / destination i; ``size`` / ``fmt``: what a destination must match."""
    if isinstance(f, DecoderFrame):
        got, row = tuple(f.shape[-2:]), (f.format, f.data, f.pitch, f.uv_offset)
    else:
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 3 or f.shape[0] != 3:
            raise TypeError('render_frames: %s %d is a (3, H, W) uint8 tensor or an ops.DecoderFrame, got %s %s'
                            % (what, i, getattr(f, 'dtype', type(f).__name__), tuple(getattr(f, 'shape', ()))))
        if not f.is_cuda:
            raise RuntimeError('render_frames: %s %d is on %s; the render kernel runs on the GPU only (no CPU fallback)' % (what, i, f.device))
        if not f.is_contiguous():
            raise TypeError('render_frames: %s %d must be contiguous' % (what, i))
        got, row = tuple(f.shape[-2:]), (0, f, 0, 0)
    if size is not None and (got != size or row[0] != fmt):
        raise ValueError('render_frames: out %d is %s of size %r, its frame %s of size %r'
                         % (i, 'planar RGB' if row[0] == 0 else 'an NV12 surface (format %d)' % row[0], got,
                            'planar RGB' if fmt == 0 else 'an NV12 surface (format %d)' % fmt, size))
    return got, row


def render_frames(frames, answers, style, luts=None, out=None):
    """frtm_render_frames_u8: the tracked objects of every frame drawn onto it, all frames in ONE launch on the current stream; nothing
    synchronises.  ``frames``: a list of (3, H, W) uint8 CUDA tensors and / or ops.DecoderFrames, any sizes; ``answers``: per frame a
    (H, W) uint8 label map of object ids, or a (K, H, W) float32 merged mask stack (what track() returns) with ``luts[i]``, its K uint8
    bytes plane -> id on the device; ``style``: an ops.RenderStyle (an NV12 frame gets its palette in the frame's own matrix and range);
    ``out``: None -- new outputs of the same kind and layout (a new DecoderFrame keeps pitch, uv_offset, matrix and range; its padding
    bytes are unspecified) --, ``frames`` itself -- in place --, or a list of the caller's surfaces, each the kind, size and format of
    its frame (pitch and uv_offset its own).  -> the list of outputs.  The arithmetic, exact in integers: include/frtm_hip.h.  The
    uploaded table of a call is kept under its rows (the last RENDER_TABLES_KEPT of them): rendering the same surfaces again uploads nothing."""
    if not isinstance(style, RenderStyle):
        raise TypeError('render_frames: style is an ops.RenderStyle, got %s' % type(style).__name__)
    frames, answers = list(frames), list(answers)
    n = len(frames)
    if not 1 <= n <= 65535:
        raise ValueError('render_frames: %d frames (1 .. 65535)' % n)
    if len(answers) != n or (luts is not None and len(luts) != n) or (out is not None and len(out) != n):
        raise ValueError('render_frames: %d frames, %d answers, %s luts, %s outputs' % (n, len(answers), luts if luts is None else len(luts),
                                                                                         out if out is None else len(out)))
    rows, outs = [], []
    for i, (f, ans) in enumerate(zip(frames, answers)):
        size, (fmt, src, pitch, uv) = _render_surface('frame', i, f)
        if not isinstance(ans, torch.Tensor) or not ((ans.dtype == torch.uint8 and ans.dim() == 2) or (ans.dtype is _F32 and ans.dim() == 3)):
            raise TypeError('render_frames: answer %d is a (H, W) uint8 label map or a (K, H, W) float32 mask stack, got %s %s'
                            % (i, getattr(ans, 'dtype', type(ans).__name__), tuple(getattr(ans, 'shape', ()))))
        if tuple(ans.shape[-2:]) != size:
            raise ValueError('render_frames: answer %d has size %r, its frame %r' % (i, tuple(ans.shape[-2:]), size))
        if not ans.is_cuda:
            raise RuntimeError('render_frames: answer %d is on %s; the render kernel runs on the GPU only (no CPU fallback)' % (i, ans.device))
        if not ans.is_contiguous():
            raise TypeError('render_frames: answer %d must be contiguous' % i)
        stack = ans.dim() == 3
        K, lut = 0, None
        if stack:
            K = ans.shape[0]
            lut = None if luts is None else luts[i]
            if not 1 <= K <= MAX_MERGE_OBJECTS + 1:
                raise ValueError('render_frames: answer %d has %d planes (1 .. %d)' % (i, K, MAX_MERGE_OBJECTS + 1))
            if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or lut.dim() != 1 or lut.numel() != K or not lut.is_cuda:
                raise TypeError('render_frames: answer %d is a stack of %d planes and needs luts[%d], %d uint8 bytes on the device' % (i, K, i, K))
        elif style.soft:
            raise ValueError('render_frames: answer %d is a label map; a soft style needs the mask stack' % i)
        if out is None:
            if isinstance(f, DecoderFrame):
                o = DecoderFrame(torch.empty(f.nbytes_needed, dtype=torch.uint8, device=f.device), f.height, f.width, pitch=f.pitch,
                                 uv_offset=f.uv_offset, matrix=f.matrix, full_range=f.full_range)
            else:
                o = torch.empty_like(f)
        else:
            o = out[i]
        _, (_, dst, dpitch, duv) = _render_surface('out', i, o, size, fmt)
        outs.append(o)
        rows.append([RENDER_FORMATS['rgb' if fmt == 0 else 'nv12'], size[0], size[1], H.ptr(src), src.numel(), pitch, uv, H.ptr(dst), dst.numel(), dpitch, duv,
                     RENDER_ANSWERS['masks' if stack else 'labels'], H.ptr(ans), ans.numel() * ans.element_size(), K, H.ptr(lut) or 0,
                     H.ptr(style.device_table(ans.device, fmt)), int(style.soft), -1 if style.edge_alpha is None else style.edge_alpha, 0])
    # a table is a function of its rows alone (they hold the addresses), so a pipeline that renders the same surfaces tick after tick --
    # a decoder's ring into an encoder's ring -- uploads each table once; fresh allocations (out=None) miss and upload
    key = (answers[0].device.index,) + tuple(v for r in rows for v in r)
    kept = _render_tables.get(key)
    if kept is None:
        host = torch.tensor(rows, dtype=torch.int64)
        kept = _render_tables[key] = (host, H.upload(host, answers[0].device))
        if len(_render_tables) > RENDER_TABLES_KEPT:
            _render_tables.popitem(last=False)
    else:
        _render_tables.move_to_end(key)
    H.call('frtm_render_frames_u8', kept[0].data_ptr(), H.ptr(kept[1]), n)
    return outs


# ----------------------------------------------------------------------------------------------------------------------
# Tracked objects measured on the device: boxes, areas, confidence in one launch (csrc/object_report.hip)
# ----------------------------------------------------------------------------------------------------------------------
OBJECT_ANSWERS = {'labels': 0, 'masks': 1}          # FRTM_OBJECT_LABELS / FRTM_OBJECT_MASKS
OBJECT_ROW_WORDS = 8                                # FRTM_OBJECT_ROW_WORDS
OBJECT_SLOTS = 16                                   # FRTM_OBJECT_SLOTS
OBJECT_WORDS = 12                                   # FRTM_OBJECT_WORDS
OBJECT_TABLES_KEPT = 256                            # uploaded row tables (with their id bytes) describe_frames keeps, least recently used first out
_object_tables = collections.OrderedDict()

ObjectStats = collections.namedtuple('ObjectStats', 'area box centroid edge border confidence soft_area')
ObjectStats.__doc__ = """One object of one frame (ObjectReport.objects): ``area`` pixels; ``box`` (x_min, y_min, x_max, y_max), inclusive, None when
the object has no pixel; ``centroid`` (x, y), None when empty; ``edge`` pixels with a 4-neighbour of another label inside the picture;
``border`` pixels on the picture's border; ``confidence`` the mean of the object's mask over its pixels, in 0 .. 1 (None for a label map or
when empty); ``soft_area`` the sum of the object's mask over the whole picture (None for a label map)."""


class ObjectReport:
    """What describe_frames measured: ``words``, the (n, 16, 12) int64 tensor of include/frtm_hip.h (on the device: making the report does
    not synchronise), with ``K[i]`` slots of frame i in use and ``stacks[i]`` True when frame i was a mask stack.  ``cpu()`` makes the one
    device-to-host copy (1.5 KB per frame) and keeps it; ``objects(i)`` -> {object id: ObjectStats} of frame i from that copy."""

    def __init__(self, words, K, stacks):
        if not isinstance(words, torch.Tensor) or words.dtype != torch.int64 or words.dim() != 3 or tuple(words.shape[1:]) != (OBJECT_SLOTS, OBJECT_WORDS):
            raise TypeError('ObjectReport: words is a (n, %d, %d) int64 tensor, got %s %s'
                            % (OBJECT_SLOTS, OBJECT_WORDS, getattr(words, 'dtype', type(words).__name__), tuple(getattr(words, 'shape', ()))))
        K, stacks = [int(k) for k in K], [bool(s) for s in stacks]
        if len(K) != words.shape[0] or len(stacks) != words.shape[0] or any(not 1 <= k <= OBJECT_SLOTS for k in K):
            raise ValueError('ObjectReport: %d frames, %d slot counts (1 .. %d), %d forms' % (words.shape[0], len(K), OBJECT_SLOTS, len(stacks)))
        self.words, self.K, self.stacks = words, K, stacks
        self._host = None

    def __len__(self):
        return self.words.shape[0]

    def cpu(self):
        if self._host is None:
            self._host = self.words.cpu()
        return self._host

    def objects(self, i):
        out = {}
        for area, x0, y0, x1, y1, sx, sy, edge, border, conf, mass, oid in self.cpu()[i, :self.K[i]].tolist():
            stack = self.stacks[i]
            out[oid] = ObjectStats(area, (x0, y0, x1, y1) if area else None, (sx / area, sy / area) if area else None, edge, border,
                                   conf / (255.0 * area) if stack and area else None, mass / 255.0 if stack else None)
        return out


def _object_ids(i, ids, who='describe_frames'):
    if isinstance(ids, (str, bytes)) or not hasattr(ids, '__len__') or not hasattr(ids, '__iter__'):
        raise TypeError(who + ': answer %d is a label map and needs ids[%d], a sequence of distinct ints in 0 .. 255, got %r' % (i, i, ids))
    ids = list(ids.tolist() if isinstance(ids, torch.Tensor) else ids)
    if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in ids):
        raise TypeError(who + ': ids[%d] holds ints, got %r' % (i, ids))
    ids = tuple(int(v) for v in ids)
    if not 1 <= len(ids) <= OBJECT_SLOTS:
        raise ValueError(who + ': ids[%d] lists %d ids (1 .. %d)' % (i, len(ids), OBJECT_SLOTS))
    if any(not 0 <= v <= 255 for v in ids):
        raise ValueError(who + ': ids[%d] is 0 .. 255, got %r' % (i, ids))
    if len(set(ids)) != len(ids):
        raise ValueError(who + ': ids[%d] lists an id twice: %r' % (i, ids))
    return ids


def _object_frames(who, answers, luts, ids):
    """The per-answer checks describe_frames and encode_frames share -> (frames: per answer (stack, h, w, tensor, K, LUT or ids), device)."""
    answers = list(answers)
    n = len(answers)
    if not 1 <= n <= 65535:
        raise ValueError(who + ': %d frames (1 .. 65535)' % n)
    if (luts is not None and len(luts) != n) or (ids is not None and len(ids) != n):
        raise ValueError(who + ': %d answers, %s luts, %s ids' % (n, luts if luts is None else len(luts), ids if ids is None else len(ids)))
    frames = []
    for i, ans in enumerate(answers):
        if not isinstance(ans, torch.Tensor) or not ((ans.dtype == torch.uint8 and ans.dim() == 2) or (ans.dtype is _F32 and ans.dim() == 3)):
            raise TypeError(who + ': answer %d is a (H, W) uint8 label map or a (K, H, W) float32 mask stack, got %s %s'
                            % (i, getattr(ans, 'dtype', type(ans).__name__), tuple(getattr(ans, 'shape', ()))))
        h, w = (int(v) for v in ans.shape[-2:])
        if not (1 <= h <= MAX_NATIVE_DIM and 1 <= w <= MAX_NATIVE_DIM):
            raise ValueError(who + ': answer %d has size %d x %d (1 .. %d)' % (i, h, w, MAX_NATIVE_DIM))
        stack = ans.dim() == 3
        if stack:
            K = int(ans.shape[0])
            lut = None if luts is None else luts[i]
            if not 1 <= K <= MAX_MERGE_OBJECTS + 1:
                raise ValueError(who + ': answer %d has %d planes (1 .. %d)' % (i, K, MAX_MERGE_OBJECTS + 1))
            if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or lut.dim() != 1 or lut.numel() != K or not lut.is_cuda:
                raise TypeError(who + ': answer %d is a stack of %d planes and needs luts[%d], %d uint8 bytes on the device' % (i, K, i, K))
            which = lut
        else:
            which = _object_ids(i, None if ids is None else ids[i], who)
            K = len(which)
        if not ans.is_cuda:
            raise RuntimeError(who + ': answer %d is on %s; the kernel runs on the GPU only (no CPU fallback)' % (i, ans.device))
        if not ans.is_contiguous():
            raise TypeError(who + ': answer %d must be contiguous' % i)
        frames.append((stack, h, w, ans, K, which))
    return frames, answers[0].device


def _object_table(frames, device):
    """The uploaded row table of ``frames`` -> (host table, device table, id bytes): a table is a function of its rows (they hold the
    addresses) and of the ids to measure, so a pipeline that describes or encodes the same buffers tick after tick uploads the table and the
    id bytes once; describe_frames and encode_frames read the same row, so they share the entries."""
    n = len(frames)
    key = (device.index,) + tuple((stack, h, w, H.ptr(ans), ans.numel() * ans.element_size(), K, H.ptr(which) if stack else which)
                                  for stack, h, w, ans, K, which in frames)
    kept = _object_tables.get(key)
    if kept is None:
        id_bytes = None
        if not all(f[0] for f in frames):
            host_ids = torch.zeros(n, OBJECT_SLOTS, dtype=torch.uint8)
            for i, (stack, _, _, _, K, which) in enumerate(frames):
                if not stack:
                    host_ids[i, :K] = torch.tensor(which, dtype=torch.uint8)
            id_bytes = H.upload(host_ids, device)
        rows = [[OBJECT_ANSWERS['masks' if stack else 'labels'], h, w, H.ptr(ans), ans.numel() * ans.element_size(), K,
                 H.ptr(which) if stack else id_bytes.data_ptr() + OBJECT_SLOTS * i, 0] for i, (stack, h, w, ans, K, which) in enumerate(frames)]
        host = torch.tensor(rows, dtype=torch.int64)
        kept = _object_tables[key] = (host, H.upload(host, device), id_bytes)
        if len(_object_tables) > OBJECT_TABLES_KEPT:
            _object_tables.popitem(last=False)
    else:
        _object_tables.move_to_end(key)
    return kept


def describe_frames(answers, luts=None, ids=None, out=None):
    """frtm_describe_frames: the objects of every frame measured -- area, box, coordinate sums, edge and border pixels, confidence and soft
    area --, all frames in ONE launch on the current stream; nothing synchronises.  ``answers``: per frame a (H, W) uint8 label map of
    object ids with ``ids[i]``, a sequence of at most 16 distinct ints in 0 .. 255 to measure (uploaded once and kept with the table), or a
    (K, H, W) float32 merged mask stack (what track() returns) with ``luts[i]``, its K uint8 bytes plane -> id on the device; any sizes,
    both kinds mixed.  ``out``: None, or an ObjectReport (or an int64 device tensor) whose buffer of at least n x 16 x 12 words is used
    again; only its first n x 16 x 12 words are written.  -> an ObjectReport.  The words, exact in integers: include/frtm_hip.h."""
    frames, device = _object_frames('describe_frames', answers, luts, ids)
    n = len(frames)
    Ks, stacks = [f[4] for f in frames], [f[0] for f in frames]
    need = n * OBJECT_SLOTS * OBJECT_WORDS
    if out is None:
        words = torch.empty(n, OBJECT_SLOTS, OBJECT_WORDS, dtype=torch.int64, device=device)
    else:
        words = out.words if isinstance(out, ObjectReport) else out
        if not isinstance(words, torch.Tensor) or words.dtype != torch.int64:
            raise TypeError('describe_frames: out is an ops.ObjectReport or an int64 tensor, got %s' % getattr(words, 'dtype', type(words).__name__))
        if not words.is_cuda:
            raise RuntimeError('describe_frames: out is on %s; the report kernel runs on the GPU only (no CPU fallback)' % (words.device,))
        if not words.is_contiguous():
            raise TypeError('describe_frames: out must be contiguous')
        if words.numel() < need:
            raise ValueError('describe_frames: out holds %d words, %d frames need %d' % (words.numel(), n, need))
    kept = _object_table(frames, device)
    H.call('frtm_describe_frames', kept[0].data_ptr(), H.ptr(kept[1]), n, H.ptr(words), words.numel())
    return ObjectReport(words.view(-1)[:need].view(n, OBJECT_SLOTS, OBJECT_WORDS), Ks, stacks)


# ----------------------------------------------------------------------------------------------------------------------
# Tracked masks coded on the device: COCO run lengths per object (csrc/mask_runs.hip)
# ----------------------------------------------------------------------------------------------------------------------
RUNS_HEAD_WORDS = 4                                 # FRTM_RUNS_HEAD_WORDS: { count, offset, area, id }
RUNS_MAX_CAPACITY = 1 << 40


class RunsOverflow(ValueError):
    """MaskRuns.cpu(): the lists need ``needed`` elements and ``runs`` holds ``capacity``; call encode again with capacity=needed."""

    def __init__(self, needed, capacity):
        ValueError.__init__(self, 'MaskRuns: the run lengths need %d elements and runs holds %d; call encode again with capacity=%d'
                            % (needed, capacity, needed))
        self.needed, self.capacity = needed, capacity


def default_run_capacity(sizes, K):
    """Elements of ``runs`` when the caller names none: per frame K (8 w + 8) -- four boundary pairs per column and slot."""
    return sum(k * (8 * w + 8) for (_, w), k in zip(sizes, K))


class MaskRuns:
    """What encode_frames coded: ``heads``, the (n, 16, 4) int64 tensor { count, offset, area, id } of include/frtm_hip.h, and ``runs``,
    the concatenated run lengths (both on the device: coding does not synchronise), with ``sizes[i]`` = (h, w) and ``K[i]`` slots of frame i
    and ``capacity``, the elements of ``runs`` the call could write.  ``runs`` is int32, not uint32 (torch's uint32 has no comparison,
    indexing or fill kernels); every count is at most h w <= 2^28, so the bits are the same.  ``cpu()`` makes the copy of the heads (512
    bytes per frame), then ONE copy of runs[:needed], and keeps both -- or raises RunsOverflow when needed > capacity; ``counts(i)`` and
    ``rle(i)`` read that copy."""

    def __init__(self, heads, runs, sizes, K, capacity):
        if not isinstance(heads, torch.Tensor) or heads.dtype != torch.int64 or heads.dim() != 3 or tuple(heads.shape[1:]) != (OBJECT_SLOTS, RUNS_HEAD_WORDS):
            raise TypeError('MaskRuns: heads is a (n, %d, %d) int64 tensor, got %s %s'
                            % (OBJECT_SLOTS, RUNS_HEAD_WORDS, getattr(heads, 'dtype', type(heads).__name__), tuple(getattr(heads, 'shape', ()))))
        if not isinstance(runs, torch.Tensor) or runs.dtype != torch.int32 or runs.dim() != 1:
            raise TypeError('MaskRuns: runs is a 1-d int32 tensor, got %s %s' % (getattr(runs, 'dtype', type(runs).__name__), tuple(getattr(runs, 'shape', ()))))
        sizes, K = [(int(h), int(w)) for h, w in sizes], [int(k) for k in K]
        if len(K) != heads.shape[0] or len(sizes) != heads.shape[0] or any(not 1 <= k <= OBJECT_SLOTS for k in K):
            raise ValueError('MaskRuns: %d frames, %d slot counts (1 .. %d), %d sizes' % (heads.shape[0], len(K), OBJECT_SLOTS, len(sizes)))
        if not 1 <= int(capacity) <= runs.numel():
            raise ValueError('MaskRuns: capacity %d of a runs of %d elements' % (capacity, runs.numel()))
        self.heads, self.runs, self.sizes, self.K, self.capacity = heads, runs, sizes, K, int(capacity)
        self._host = None

    def __len__(self):
        return self.heads.shape[0]

    def cpu(self):
        """-> (heads, runs[:needed]) on the host; two copies the first time, none after."""
        if self._host is None or self._host[1] is None:
            heads = self.heads.cpu() if self._host is None else self._host[0]
            self._host = (heads, None)
            count, offset = heads[-1, self.K[-1] - 1, :2].tolist()
            if offset + count > self.capacity:
                raise RunsOverflow(offset + count, self.capacity)
            self._host = (heads, self.runs[:offset + count].cpu())
        return self._host

    def counts(self, i):
        """-> {object id: the list of run lengths of the object's mask in frame i}."""
        heads, runs = self.cpu()
        return {oid: runs[offset:offset + count].tolist() for count, offset, _, oid in heads[i, :self.K[i]].tolist()}

    def rle(self, i, compressed=False):
        """-> {object id: {'size': [h, w], 'counts': list -- or bytes, COCO's string form, when ``compressed``}}."""
        return {oid: {'size': list(self.sizes[i]), 'counts': rle_to_string(c) if compressed else c} for oid, c in self.counts(i).items()}


def rle_to_string(counts):
    """COCO's string form of a list of run lengths: from the fourth count on the difference to the count two before is coded; a value goes out
    in 5-bit groups, low first, bit 0x20 marks 'more', and it is finished when the rest is 0 with bit 0x10 clear or -1 with bit 0x10 set;
    every group + 48 is a character.  (A restatement of the coder of the COCO API, not a call into it.)"""
    counts = [int(c) for c in counts]
    out = bytearray()
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5                                 # (arithmetic: a negative rest ends at -1)
            more = x != -1 if c & 0x10 else x != 0
            out.append((c | 0x20 if more else c) + 48)
    return bytes(out)


def rle_from_string(s):
    """The list of run lengths of COCO's string form (rle_to_string's inverse)."""
    s = bytes(s.encode('ascii') if isinstance(s, str) else s)
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            if p >= len(s):
                raise ValueError('rle_from_string: the string ends inside a value')
            c = s[p] - 48
            if not 0 <= c < 64:
                raise ValueError('rle_from_string: byte %d at %d is no character of the code' % (s[p], p))
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p, k = p + 1, k + 1
            if not more and c & 0x10:
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_decode(size, counts):
    """The (h, w) numpy bool mask of a list of run lengths (or of its string form): runs of zeros and ones in turn, column-major."""
    import numpy as np
    h, w = (int(v) for v in size)
    counts = rle_from_string(counts) if isinstance(counts, (bytes, str)) else [int(c) for c in counts]
    if any(c < 0 for c in counts) or sum(counts) != h * w:
        raise ValueError('rle_decode: the counts sum to %d, the size is %d x %d' % (sum(counts), h, w))
    bits = np.zeros(len(counts), dtype=bool)
    bits[1::2] = True
    return np.repeat(bits, counts).reshape(w, h).T


def encode_frames(answers, luts=None, ids=None, out=None, capacity=None):
    """frtm_encode_frames: every object's mask of every frame as COCO run lengths (column-major, starting with a run of zeros), all frames in
    FOUR launches on the current stream whatever their number, sizes and content; nothing synchronises.  ``answers``, ``luts``, ``ids``:
    describe_frames's arguments and checks (the two calls share the uploaded table).  ``capacity``: the elements of ``runs``; default: the
    sum over the frames of K (8 w + 8), or what ``out`` holds.  ``out``: a MaskRuns whose buffers (at least n x 16 x 4 words, and
    ``capacity`` elements) are used again; only the first n x 16 x 4 words and min(needed, capacity) elements are written.  -> a MaskRuns;
    its heads hold the true counts and offsets even when the lists did not fit (MaskRuns.cpu() then raises RunsOverflow with ``needed``).
    The workspace comes from ops.workspace.  The format, exact in integers: include/frtm_hip.h."""
    frames, device = _object_frames('encode_frames', answers, luts, ids)
    n = len(frames)
    Ks, sizes = [f[4] for f in frames], [(f[1], f[2]) for f in frames]
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, numbers.Integral) or not 1 <= capacity <= RUNS_MAX_CAPACITY):
        raise ValueError('encode_frames: capacity is 1 .. 2^40 elements, got %r' % (capacity,))
    need = n * OBJECT_SLOTS * RUNS_HEAD_WORDS
    if out is None:
        capacity = default_run_capacity(sizes, Ks) if capacity is None else int(capacity)
        heads = torch.empty(n, OBJECT_SLOTS, RUNS_HEAD_WORDS, dtype=torch.int64, device=device)
        runs = torch.empty(capacity, dtype=torch.int32, device=device)
    else:
        if not isinstance(out, MaskRuns):
            raise TypeError('encode_frames: out is an ops.MaskRuns, got %s' % type(out).__name__)
        heads, runs = out.heads, out.runs
        if not heads.is_cuda or not runs.is_cuda:
            raise RuntimeError('encode_frames: out is on %s; the kernel runs on the GPU only (no CPU fallback)' % (heads.device,))
        if not heads.is_contiguous() or not runs.is_contiguous():
            raise TypeError('encode_frames: out must be contiguous')
        if heads.numel() < need:
            raise ValueError('encode_frames: out holds %d head words, %d frames need %d' % (heads.numel(), n, need))
        capacity = runs.numel() if capacity is None else int(capacity)
        if capacity > runs.numel():
            raise ValueError('encode_frames: capacity %d, out holds %d elements' % (capacity, runs.numel()))
    kept = _object_table(frames, device)
    L = H.lib()
    work_bytes = L.frtm_encode_work_bytes(kept[0].data_ptr(), n, capacity)
    if work_bytes == 0:
        raise RuntimeError('frtm_encode_work_bytes failed: %s' % L.frtm_last_error().decode())
    work = workspace(device, (work_bytes + 3) // 4)
    H.call('frtm_encode_frames', kept[0].data_ptr(), H.ptr(kept[1]), n, H.ptr(heads), heads.numel(), H.ptr(runs), capacity, H.ptr(work),
           work.numel() * work.element_size())
    return MaskRuns(heads.view(-1)[:need].view(n, OBJECT_SLOTS, RUNS_HEAD_WORDS), runs, sizes, Ks, capacity)


# ----------------------------------------------------------------------------------------------------------------------
# The answer cleaned on the device: connected parts, specks dropped (csrc/object_parts.hip)
# ----------------------------------------------------------------------------------------------------------------------
PARTS_ROW_WORDS = 16                                # FRTM_PARTS_ROW_WORDS
PARTS_WORDS = 12                                    # FRTM_PARTS_WORDS
PARTS_TILE_H = 32                                   # FRTM_PARTS_TILE_H
PARTS_TILE_W = 64                                   # FRTM_PARTS_TILE_W: the tile of the local pass; its sides are the seams
PARTS_MAX_MIN_AREA = 1 << 28
PARTS_TABLES_KEPT = 256                             # uploaded row tables clean_frames keeps, least recently used first out
_parts_tables = collections.OrderedDict()

PartStats = collections.namedtuple('PartStats', 'parts kept area kept_area largest_area largest_box largest_name ruled')
PartStats.__doc__ = """One object of one frame (CleanedAnswers.objects): ``parts`` connected parts, ``kept`` of them kept; ``area`` pixels,
``kept_area`` of them kept; ``largest_area``, ``largest_box`` (x_min, y_min, x_max, y_max), inclusive, and ``largest_name`` (the smallest
y w + x among its pixels) of the largest part, ties to the smaller name -- box and name None when the object has no pixel; ``ruled`` False
when the object's id is ``fill`` (the background: counted, all kept)."""


def clean_work_bytes(h, w):
    """A frame's part of clean_frames's work buffer: 16 packed words, then two int32 per pixel, a multiple of 16 bytes
    (frtm_clean_work_bytes is the sum over the frames)."""
    return (128 + 8 * h * w + 15) // 16 * 16


class CleanedAnswers:
    """What clean_frames made: ``labels[i]``, the (h, w) uint8 cleaned label map of frame i (a view of one packed buffer, every frame on a
    16-byte boundary); ``components[i]``, the (h, w) int32 map of part names (-1: no slot), or None when not asked for; ``words``, the
    (n, 16, 12) int64 tensor of include/frtm_hip.h; ``status``, n int64 words behind it -- all on the device: cleaning does not
    synchronise.  ``cpu()`` makes ONE device-to-host copy of words and status and keeps it; it raises RuntimeError naming the frame whose
    status is not 0.  ``objects(i)`` -> {object id: PartStats}; ``ids(i)``: the ids to pass on with ``labels[i]``; ``answers()`` ->
    (labels, ids) for describe_frames / encode_frames / render_frames."""

    def __init__(self, label_buf, comp_buf, word_buf, sizes, K, ids):
        sizes, K = [(int(h), int(w)) for h, w in sizes], [int(k) for k in K]
        n = len(sizes)
        if len(K) != n or len(ids) != n or n < 1 or any(not 1 <= k <= OBJECT_SLOTS for k in K):
            raise ValueError('CleanedAnswers: %d sizes, %d slot counts (1 .. %d), %d id lists' % (n, len(K), OBJECT_SLOTS, len(ids)))
        if not isinstance(word_buf, torch.Tensor) or word_buf.dtype != torch.int64 or word_buf.dim() != 1 or word_buf.numel() < n * (OBJECT_SLOTS * PARTS_WORDS + 1):
            raise TypeError('CleanedAnswers: the words are a 1-d int64 tensor of at least %d x (%d x %d + 1) elements, got %s %s'
                            % (n, OBJECT_SLOTS, PARTS_WORDS, getattr(word_buf, 'dtype', type(word_buf).__name__), tuple(getattr(word_buf, 'shape', ()))))
        if not isinstance(label_buf, torch.Tensor) or label_buf.dtype != torch.uint8 or label_buf.dim() != 1:
            raise TypeError('CleanedAnswers: the label maps are a 1-d uint8 tensor, got %s' % getattr(label_buf, 'dtype', type(label_buf).__name__))
        if comp_buf is not None and (not isinstance(comp_buf, torch.Tensor) or comp_buf.dtype != torch.int32 or comp_buf.dim() != 1):
            raise TypeError('CleanedAnswers: the component maps are a 1-d int32 tensor or None, got %s' % getattr(comp_buf, 'dtype', type(comp_buf).__name__))
        offs, o = [], 0
        for h, w in sizes:
            offs.append(o)
            o += (h * w + 15) // 16 * 16
        if label_buf.numel() < o or (comp_buf is not None and comp_buf.numel() < o):
            raise ValueError('CleanedAnswers: the frames need %d packed pixels, the buffers hold %d and %s'
                             % (o, label_buf.numel(), None if comp_buf is None else comp_buf.numel()))
        self.label_buf, self.comp_buf, self.word_buf = label_buf, comp_buf, word_buf
        self.sizes, self.K, self.offsets, self.pixels = sizes, K, offs, o
        self._ids = [None if v is None else tuple(int(x) for x in v) for v in ids]
        nw = n * OBJECT_SLOTS * PARTS_WORDS
        self.words = word_buf[:nw].view(n, OBJECT_SLOTS, PARTS_WORDS)
        self.status = word_buf[nw:nw + n]
        self.labels = [label_buf[a:a + h * w].view(h, w) for a, (h, w) in zip(offs, sizes)]
        self.components = [None if comp_buf is None else comp_buf[a:a + h * w].view(h, w) for a, (h, w) in zip(offs, sizes)]
        self._host = None

    def __len__(self):
        return len(self.sizes)

    def cpu(self):
        """-> (words, status) on the host; one copy the first time, none after.  RuntimeError when a frame's status is not 0."""
        if self._host is None:
            n = len(self)
            nw = n * OBJECT_SLOTS * PARTS_WORDS
            host = self.word_buf[:nw + n].cpu()
            self._host = (host[:nw].view(n, OBJECT_SLOTS, PARTS_WORDS), host[nw:])
        bad = [(i, s) for i, s in enumerate(self._host[1].tolist()) if s != 0]
        if bad:
            raise RuntimeError('CleanedAnswers: frame %d has status %d: a bounded loop of the labelling gave up (1 local, 2 seam, 4 flatten); '
                               'its outputs are not valid' % bad[0])
        return self._host

    def objects(self, i):
        out = {}
        for parts, kept, area, kept_area, big, name, x0, y0, x1, y1, ruled, oid in self.cpu()[0][i, :self.K[i]].tolist():
            out[oid] = PartStats(parts, kept, area, kept_area, big, (x0, y0, x1, y1) if area else None, name if area else None, bool(ruled))
        return out

    def ids(self, i):
        """The ids that go with ``labels[i]``: what the caller listed (a label map's ids, a stack's plane_ids) -- no copy --, else word 11
        of the frame's slots from cpu()."""
        if self._ids[i] is None:
            self._ids[i] = tuple(self.cpu()[0][i, :self.K[i], 11].tolist())
        return self._ids[i]

    def answers(self):
        """-> (labels, ids): ``ops.describe_frames(labels, ids=ids)``, ``ops.encode_frames(labels, ids=ids)``."""
        return list(self.labels), [self.ids(i) for i in range(len(self))]


def _parts_rule(who, connectivity, min_area, largest_only, fill):
    for name, v in (('connectivity', connectivity), ('min_area', min_area), ('fill', fill)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise TypeError('%s: %s is an int, got %r' % (who, name, v))
    if connectivity not in (4, 8):
        raise ValueError('%s: connectivity is 4 or 8, got %r' % (who, connectivity))
    if not 1 <= min_area <= PARTS_MAX_MIN_AREA:
        raise ValueError('%s: min_area is 1 .. 2^28, got %r' % (who, min_area))
    if not isinstance(largest_only, (bool, numbers.Integral)) or largest_only not in (0, 1):
        raise ValueError('%s: largest_only is a bool, got %r' % (who, largest_only))
    if not 0 <= fill <= 255:
        raise ValueError('%s: fill is 0 .. 255, got %r' % (who, fill))
    return int(connectivity), int(min_area), int(bool(largest_only)), int(fill)


def clean_frames(answers, luts=None, ids=None, connectivity=8, min_area=1, largest_only=False, fill=0, components=False, plane_ids=None,
                 out=None):
    """frtm_clean_frames: every object of every frame split into its connected parts (``connectivity`` 4 or 8), the parts measured, and a
    cleaned uint8 label map written per frame, all frames in SIX launches on the current stream whatever their number, sizes and content;
    nothing synchronises.  ``answers``, ``luts``, ``ids``: describe_frames's arguments and checks.  The rule: an object whose id is not
    ``fill`` keeps the parts of at least ``min_area`` pixels -- with ``largest_only`` only its largest part, ties to the part that starts
    first --; every other pixel of it becomes ``fill``; the object whose id is ``fill`` (the background) is counted and left as it is.
    ``components``: also write the int32 map of part names.  ``plane_ids[i]``: the ids of a stack's planes when the caller knows them on the
    host (then CleanedAnswers.ids needs no copy).  ``out``: a CleanedAnswers whose buffers are used again when they are large enough;
    only the frames' own pixels and words are written.  -> a CleanedAnswers.  The workspace comes from ops.workspace.  The parts, the rule
    and the words, exact in integers: include/frtm_hip.h.  Not done here: filling holes, giving removed pixels a neighbour's label,
    opening or closing, feeding the map back into the tracker, a confidence for the cleaned map."""
    who = 'clean_frames'
    frames, device = _object_frames(who, answers, luts, ids)
    n = len(frames)
    connectivity, min_area, largest_only, fill = _parts_rule(who, connectivity, min_area, largest_only, fill)
    if plane_ids is not None and len(plane_ids) != n:
        raise ValueError('%s: %d answers, %d plane_ids' % (who, n, len(plane_ids)))
    Ks, sizes = [f[4] for f in frames], [(f[1], f[2]) for f in frames]
    host_ids = []
    for i, (stack, _, _, _, K, which) in enumerate(frames):
        known = which if not stack else None if plane_ids is None or plane_ids[i] is None else _object_ids(i, plane_ids[i], who)
        if known is not None and len(known) != K:
            raise ValueError('%s: plane_ids[%d] lists %d ids, the stack has %d planes' % (who, i, len(known), K))
        host_ids.append(known)
    pixels = sum((h * w + 15) // 16 * 16 for h, w in sizes)
    n_words = n * (OBJECT_SLOTS * PARTS_WORDS + 1)
    if out is None:
        label_buf = torch.empty(pixels, dtype=torch.uint8, device=device)
        comp_buf = torch.empty(pixels, dtype=torch.int32, device=device) if components else None
        word_buf = torch.empty(n_words, dtype=torch.int64, device=device)
    else:
        if not isinstance(out, CleanedAnswers):
            raise TypeError('%s: out is an ops.CleanedAnswers, got %s' % (who, type(out).__name__))
        label_buf, comp_buf, word_buf = out.label_buf, out.comp_buf if components else None, out.word_buf
        if not label_buf.is_cuda or not word_buf.is_cuda or (comp_buf is not None and not comp_buf.is_cuda):
            raise RuntimeError('%s: out is on %s; the kernels run on the GPU only (no CPU fallback)' % (who, label_buf.device))
        if components and comp_buf is None:
            raise ValueError('%s: components asked for, out holds no component maps' % who)
        if label_buf.numel() < pixels or word_buf.numel() < n_words or (comp_buf is not None and comp_buf.numel() < pixels):
            raise ValueError('%s: out holds %d pixels and %d words, %d frames need %d and %d' % (who, label_buf.numel(), word_buf.numel(), n, pixels, n_words))
    kept = _object_table(frames, device)
    L = H.lib()
    first = torch.zeros(n, PARTS_ROW_WORDS, dtype=torch.int64)
    first[:, :OBJECT_ROW_WORDS] = kept[0]
    work_bytes = L.frtm_clean_work_bytes(first.data_ptr(), n)
    if work_bytes == 0:
        raise RuntimeError('frtm_clean_work_bytes failed: %s' % L.frtm_last_error().decode())
    work = workspace(device, (work_bytes + 15) // 4 + 4)
    base = (H.ptr(work) + 15) // 16 * 16
    key = (device.index, H.ptr(label_buf), None if comp_buf is None else H.ptr(comp_buf), base) + tuple(tuple(r) for r in kept[0].tolist())
    table = _parts_tables.get(key)
    if table is None:
        o = wo = 0
        for i, (h, w) in enumerate(sizes):
            first[i, OBJECT_ROW_WORDS:] = torch.tensor([H.ptr(label_buf) + o, h * w, 0 if comp_buf is None else H.ptr(comp_buf) + 4 * o,
                                                        0 if comp_buf is None else 4 * h * w, base + wo, clean_work_bytes(h, w), 0, 0], dtype=torch.int64)
            o += (h * w + 15) // 16 * 16
            wo += clean_work_bytes(h, w)
        table = _parts_tables[key] = (first, H.upload(first, device), kept)
        if len(_parts_tables) > PARTS_TABLES_KEPT:
            _parts_tables.popitem(last=False)
    else:
        _parts_tables.move_to_end(key)
    nw = n * OBJECT_SLOTS * PARTS_WORDS
    H.call('frtm_clean_frames', table[0].data_ptr(), H.ptr(table[1]), n, connectivity, min_area, largest_only, fill, H.ptr(word_buf), nw,
           H.ptr(word_buf) + 8 * nw, n)
    return CleanedAnswers(label_buf, comp_buf, word_buf, sizes, Ks, host_ids)
