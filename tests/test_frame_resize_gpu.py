"""The batched resize kernels on the GPU (csrc/frame_resize.hip) against the fp64 restatements of tests/_frame_refs.py, torch's bicubic
and nearest operators, and through DeviceFrameResizer into one training step on files.

Criterion for frames (R.assert_band): equal to the half-even rounding of the fp64 value wherever that value's fractional part is farther
than 1e-3 from 0.5 -- an fp32 sum of a normalised mean of values <= 255 with weights one rounding from exact cannot move it that far --
and at most 1 LSB off elsewhere.  The band is a cap, not a measurement: for every frame of non-integer ratio the share of outputs
inside it is asserted, on the fp64 reference alone, to be below 1 % (uniform fractions: 0.2 %).  Labels must equal torch exactly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _file_trees as trees
import _frame_refs as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _pack(frames, last):
    """Frames back to back, no padding -> (flat uint8 tensor, CPU int64 table)."""
    rows, off = [], 0
    for f, v in zip(frames, last):
        rows.append((off, f.shape[-2], f.shape[-1], v))
        off += f.size
    return torch.from_numpy(np.concatenate([f.ravel() for f in frames])), torch.tensor(rows, dtype=torch.int64)


def _resize(frames, shapes, size):
    from frtm_vos_amd import ops
    src, table = _pack(frames, [ops.RESIZE_MODES[m] for _, _, m in shapes])
    return ops.resize_frames_u8(src.to(DEV), table, frames[0].shape[0], size), src, table


@pytest.fixture(scope='module')
def mixed():
    frames = R.seeded_frames(R.MIXED, 11)
    out, src, table = _resize(frames, R.MIXED, R.TARGET)
    assert sum(int(o) % 2 for o in table[:, 0]) >= 3 and sum(int(o) % 16 != 0 for o in table[:, 0]) >= 5      # misaligned bases
    return frames, out, src, table


def _check(shapes, frames, out, capped, size=R.TARGET):
    out = out.cpu().numpy()
    for k, (shape, frame) in enumerate(zip(shapes, frames)):
        ref = R.resize_ref(frame, size, shape[2])
        mism, share = R.assert_band(out[k], ref, str(shape))
        print('%s: %d of %d outputs differ (all inside the near-tie band), band share %.4f' % (shape, mism, ref.size, share))
        if k in capped:
            assert share < R.BAND_CAP, (shape, share)


def test_area_mixed_call(mixed):
    frames, out, _, _ = mixed
    assert out.dtype == torch.uint8 and tuple(out.shape) == (7, 3) + R.TARGET and out.device == torch.device(DEV)
    _check(R.MIXED, frames, out, R.CAPPED_MIXED)
    got = out.cpu().numpy()
    assert np.array_equal(got[R.IDENTITY], frames[R.IDENTITY])                                    # a frame already at the target size
    f = frames[R.RATIO2].astype(np.int64)
    exact = (f[:, 0::2, 0::2] + f[:, 0::2, 1::2] + f[:, 1::2, 0::2] + f[:, 1::2, 1::2]) / 4.0     # every fp32 operation is exact here
    assert np.array_equal(got[R.RATIO2], np.rint(exact).astype(np.uint8))


def test_cubic_against_torch(mixed):
    frames, out, _, _ = mixed
    x = torch.from_numpy(frames[R.CUBIC].astype(np.float64))[None]
    ref = F.interpolate(x, R.TARGET, mode='bicubic', align_corners=False)[0].numpy()
    mism, share = R.assert_band(out[R.CUBIC].cpu().numpy(), ref, 'cubic 20 x 30')
    print('cubic: %d outputs differ inside the band, band share %.4f' % (mism, share))
    assert share < R.BAND_CAP and float(ref.min()) < 0 and float(ref.max()) > 255                 # the clamp is exercised


def test_extra_frames_column_chunks_and_thin_sources():
    frames = R.seeded_frames(R.EXTRA, 12)
    out, _, _ = _resize(frames, R.EXTRA, R.TARGET)
    _check(R.EXTRA, frames, out, R.CAPPED_EXTRA)
    k = R.EXACT_EXTRA                                                                             # 68 -> 51: weights 3/4, 1/4, 1/2, exact sums
    assert np.array_equal(out[k].cpu().numpy(), R.round_u8(R.resize_ref(frames[k], R.TARGET, 'area')))


def test_real_size_frame():
    shapes = [(720, 1280, 'area')]
    frames = R.seeded_frames(shapes, 13)
    out, _, _ = _resize(frames, shapes, (480, 854))
    _check(shapes, frames, out, [0], size=(480, 854))


def test_second_call_is_bit_identical(mixed):
    from frtm_vos_amd import ops
    _, out, src, table = mixed
    again = ops.resize_frames_u8(src.to(DEV), table, 3, R.TARGET)
    assert torch.equal(out, again)


@pytest.mark.parametrize('size', [R.TARGET, (480, 854)], ids=lambda s: '%dx%d' % s)
def test_labels_equal_torch_nearest(size):
    from frtm_vos_amd import ops
    rng = np.random.default_rng(14)
    maps = [rng.choice(np.array([0, 1, 2, 5], dtype=np.uint8), (1, h, w)) for h, w in ((45, 77), (30, 51), (720, 1280))]
    src, table = _pack(maps, [2, 2, 2])
    out = ops.resize_labels_u8(src.to(DEV), table, size)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, 1) + size
    for k, m in enumerate(maps):
        want = F.interpolate((torch.from_numpy(m)[None] == 2).float(), size, mode='nearest').byte()[0]
        assert torch.equal(out[k].cpu(), want), m.shape
        assert np.array_equal(want[0].numpy(), R.label_ref(m[0], 2, size))
    assert torch.equal(out, ops.resize_labels_u8(src.to(DEV), table, size))
    other = ops.resize_labels_u8(src.to(DEV), torch.tensor([[0, 45, 77, 5]]), size)                # another id, first map only
    assert torch.equal(other[0].cpu(), F.interpolate((torch.from_numpy(maps[0])[None] == 5).float(), size, mode='nearest').byte()[0])


def test_bad_arguments_return_err_arg():
    from frtm_vos_amd import _hip, ops
    L = _hip.lib()
    src = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 3, 30, 51), 7, dtype=torch.uint8, device=DEV)

    def call(entry, row, H=30, W=51, planes=(3,)):
        host = torch.tensor([row], dtype=torch.int64)
        dev = host.to(DEV)
        return getattr(L, entry)(src.data_ptr(), src.numel(), host.data_ptr(), dev.data_ptr(), 1, *planes, out.data_ptr(), H, W, _hip.stream())
    for row in ((0, 0, 20, 0), (0, 10, 0, 0), (0, 10, 20, 2), (0, 10, 20, -1), (4000, 10, 20, 0)):
        assert call('frtm_resize_frames_u8', row) == -1, row
    assert call('frtm_resize_frames_u8', (0, 10, 20, 0), H=0) == -1 and call('frtm_resize_frames_u8', (0, 10, 20, 0), W=0) == -1
    for row in ((0, 0, 20, 2), (0, 10, 0, 2), (0, 10, 20, 256), (4000, 10, 20, 2)):
        assert call('frtm_resize_labels_u8', row, planes=()) == -1, row
    assert call('frtm_resize_labels_u8', (0, 10, 20, 2), H=0, planes=()) == -1
    torch.cuda.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7                                            # nothing was launched
    with pytest.raises(RuntimeError, match=r'frtm_resize_frames_u8 failed \(-1\)'):
        ops.resize_frames_u8(src, torch.tensor([[0, 10, 20, 3]]), 3, R.TARGET)
    assert call('frtm_resize_frames_u8', (0, 10, 20, 0)) == 0                                     # the same call with a valid row runs


# ---- through the sample sets ----
@pytest.fixture(scope='module')
def ytvos_batch(tmp_path_factory):
    from frtm_vos_amd.lib.training_datasets import YouTubeVOSDataset, raw_collate
    root = trees.make_ytvos(tmp_path_factory.mktemp('ytvos'))
    y = YouTubeVOSDataset(root, epoch_samples=0, meta_file=root / 'meta.pth')
    pick = [i for i, s in enumerate(y.specs) if (s.seq_name, s.obj_id) in (('0a1b2c', 3), ('3d4e5f', 1))]      # landscape and portrait
    return y, raw_collate([y[i] for i in pick])


def test_device_frame_resizer_equals_the_per_frame_kernels(ytvos_batch):
    from frtm_vos_amd import ops
    from frtm_vos_amd.lib.training_datasets import DeviceFrameResizer
    from frtm_vos_amd.model.training_model import SampleSpec
    y, batch = ytvos_batch
    size = (64, 96)
    resize = DeviceFrameResizer(size, DEV, datasets=[y])
    images, labels, meta = resize(batch)
    specs = SampleSpec.from_encoded(meta)
    assert meta == batch[2] and len(images) == len(labels) == 3
    for t in range(3):
        assert images[t].dtype == labels[t].dtype == torch.uint8 and images[t].device == labels[t].device == torch.device(DEV)
        assert tuple(images[t].shape) == (2, 3) + size and tuple(labels[t].shape) == (2, 1) + size
        assert images[t].is_contiguous() and labels[t].is_contiguous()
        for b, spec in enumerate(specs):
            im, lb = batch[0][t][b], batch[1][t][b]
            assert resize.mode(spec.seq_name, im.shape[1]) == 'cubic'                             # 40 and 48 rows enlarged to 64
            one = ops.resize_frames_u8(im.reshape(-1).to(DEV), torch.tensor([[0, im.shape[1], im.shape[2], ops.RESIZE_MODES['cubic']]]), 3, size)
            assert torch.equal(images[t][b], one[0])
            R.assert_band(one[0].cpu().numpy(), R.resize_ref(im.numpy(), size, 'cubic'), 'resizer frame')
            want = F.interpolate((lb[None] == spec.obj_id).float(), size, mode='nearest').byte()[0]
            assert torch.equal(labels[t][b].cpu(), want) and int(want.sum()) > 0
    # a DAVIS sample set's frames take 'area' whatever their size; here: reduced to 30 x 51
    small = DeviceFrameResizer(R.TARGET, DEV)
    small.area_sequences = {s.seq_name for s in specs}
    im = batch[0][0][0]
    got = small(batch)[0][0][0]
    R.assert_band(got.cpu().numpy(), R.resize_ref(im.numpy(), R.TARGET, 'area'), 'area through the resizer')
    again = resize(batch)                                                                         # the staging buffers are reused
    assert all(torch.equal(a, b) for a, b in zip(images + labels, again[0] + again[1]))


def test_training_step_on_files(ytvos_batch, tmp_path):
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.fused_adam import FusedAdam
    from frtm_vos_amd.lib.training_datasets import DeviceFrameResizer
    from frtm_vos_amd.model.augmenter import ImageAugmenter
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    from frtm_vos_amd.model.seg_network import SegNetwork
    from frtm_vos_amd.model.training_model import TrainerModel
    y, batch = ytvos_batch
    P = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18')
    P.disc_params.update(memory_size=20, init_iters=(3, 5), update_iters=(3,), c_channels=32)
    ext = ResnetFeatureExtractor('resnet18').to(DEV)
    chans = {L: c for L, c in ext.get_out_channels().items() if L in P.refnet_params.layers}
    torch.manual_seed(1)
    refiner = SegNetwork(1, 64, chans, True).to(DEV)
    model = TrainerModel(ImageAugmenter(P.aug_params), ext, P.disc_params, refiner, batch_size=2,
                         tmodel_cache=dict(path=tmp_path / 'cache', enable=True, read_only=False), device=DEV, refiner_backend='hip',
                         loss_backend='hip')
    opt = FusedAdam(refiner.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-5, amsgrad=True)
    before = [p.detach().clone() for p in refiner.parameters()]
    np.random.seed(0)
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    try:
        opt.zero_grad()
        stats = model(*DeviceFrameResizer((128, 160), DEV, datasets=[y])(batch))
        opt.step()
    finally:
        torch.set_grad_enabled(prev)
    print(stats)
    assert stats['stats/fcache_hits'] == 0 and np.isfinite(stats['stats/loss']) and stats['stats/loss'] > 0
    assert 0 <= stats['stats/accuracy'] <= 1
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in refiner.parameters())
    assert all(bool(torch.isfinite(p).all()) for p in refiner.parameters())
    assert sum(not torch.equal(a, b) for a, b in zip(before, refiner.parameters())) > 100
    assert sorted(p.name for p in (tmp_path / 'cache').iterdir()) == ['0a1b2c', '3d4e5f']          # target models stored under the sample's identity
