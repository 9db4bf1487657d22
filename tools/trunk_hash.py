"""sha256 of the five trunk taps for a few frame sizes in every precision mode, with the pass's FLOP ledgers and launch count, for an A/B of two builds
of the library (or of a switch) that must not change a bit:  python tools/trunk_hash.py [path/to/libfrtm_hip.so]   (one process per library; diff the
outputs).  The last block runs small frames under FRTM_BF16X1_MIN_COLS=0, so that every bf16 route is taken there as well.  The kernels are
deterministic and the ledgers are sums of exact integers, so one unequal character is a changed route or order of operations, not noise."""
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from frtm_vos_amd import _hip as H  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
if args:
    H.LIB_PATH = os.path.abspath(args[0])          # before the first call loads it
for name in [n for n in H.SIGNATURES if not hasattr(ctypes.CDLL(H.LIB_PATH), n)]:          # an older build (before frtm_backbone_conv_route): bind what it has
    del H.SIGNATURES[name]
from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor  # noqa: E402

MODES = ('fp32', 'bf16x3', 'bf16x1', 'bf16x1_3x3')
CASES = (('resnet101', (480, 854), 3), ('resnet101', (480, 854), 8), ('resnet18', (75, 101), 2), ('resnet50', (96, 128), 1), ('resnet18', (33, 258), 2),
         ('resnet18', (64, 39), 1))
ROUTED = (('resnet101', (96, 160), 2), ('resnet18', (75, 101), 2), ('resnet50', (96, 128), 1))          # under FRTM_BF16X1_MIN_COLS=0


def run(cases, label):
    for name, size, B in cases:
        ext = ResnetFeatureExtractor(name).to('cuda:0')
        img = torch.randint(0, 256, (B, 3) + size, dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to('cuda:0')
        for mode in MODES:
            ext.precision = mode
            out = ext(img)
            torch.cuda.synchronize()
            print(label, name, size, B, mode, ' '.join(hashlib.sha256(out[L].cpu().numpy().tobytes()).hexdigest()[:12] for L in out),
                  'flops %r executed %r forms %r launches %d' % (ext.last_flops, ext.last_flops_executed, ext.last_flops_form, ext.last_conv_launches))
        del ext


with torch.no_grad():
    H.lib()
    print('library:', [ln.split()[-1] for ln in open('/proc/self/maps') if 'libfrtm_hip' in ln][0], file=sys.stderr)      # (stderr: the outputs stay comparable)
    run(CASES, 'table')
    os.environ['FRTM_BF16X1_MIN_COLS'] = '0'          # read when a trunk is created
    run(ROUTED, 'min_cols=0')
