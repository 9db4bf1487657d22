"""tools/make_golden_g19.py -- TEST INFRASTRUCTURE; runs only where the upstream reference is checked out (it imports the reference's own
modules through oracle/ref_harness.py, read-only; nothing under oracle/ is edited).

    python tools/make_golden_g19.py            # writes tests/golden/g19_upsampler.npz

Records the refiner of the reference's YouTube-VOS fork, whose head is the bicubic ``Upsampler`` (ytvos_validation/seg_network.py:62-75,101):
  A_* / B_*   ``ytvos_validation.seg_network.SegNetwork`` on name-seeded weights (oracle.make_golden.keyed_state_dict), BatchNorm on, eval mode,
              the small widths of fixture G7 (layer5..layer2 = 32/16/8/8, out_channels 8); one call per object (the fork takes `scores` as a
              list).  Two image sizes whose final resize ratio is not an integer: A 56x90 from a 13x21 layer2 map (2x: 26x42, ratio ~2.15) and
              B 40x58 from a 14x19 layer2 map (2x: 28x38, ratio ~1.5).
  up_*        the main reference's ``model.seg_network.Upsampler`` alone (model/seg_network.py:59-72) on one random input.
Inputs and outputs only; the weights are rebuilt from their key names on the other side.
"""
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as R                       # noqa: E402,F401  (refuses to load without the reference)
from oracle.make_golden import keyed_state_dict            # noqa: E402

sys.modules.setdefault('easydict', types.ModuleType('easydict'))
from ytvos_validation import seg_network as YS             # noqa: E402  (the fork's refiner)
from model import seg_network as MS                        # noqa: E402  (the main reference's refiner module)

CHANS = OrderedDict(layer5=32, layer4=16, layer3=8, layer2=8)
CASES = {'A': ((56, 90), [(2, 3), (4, 6), (7, 11), (13, 21)], 2),
         'B': ((40, 58), [(2, 3), (4, 5), (7, 10), (14, 19)], 3)}


def main():
    res = {}
    net = YS.SegNetwork(1, 8, CHANS, True).eval()
    net.load_state_dict(keyed_state_dict(net))
    res['nkeys'] = len(net.state_dict())
    for tag, (size, dims, n_obj) in CASES.items():
        g = torch.Generator().manual_seed(190 + ord(tag))
        feats = {L: torch.randn(1, c, *d, generator=g) for (L, c), d in zip(CHANS.items(), dims)}
        scores = torch.randn(n_obj, 1, *dims[1], generator=g)
        with torch.no_grad():
            out = torch.cat([net([scores[k:k + 1]], feats, size) for k in range(n_obj)])     # one object per call
        assert out.shape == (n_obj, 1) + size
        for L, t in feats.items():
            res['%s_ft_%s' % (tag, L)] = t
        res[tag + '_scores'] = scores
        res[tag + '_size'] = np.array(size)
        res[tag + '_out'] = out
    up = MS.Upsampler(16).eval()
    up.load_state_dict(keyed_state_dict(up))
    g = torch.Generator().manual_seed(191)
    x = torch.randn(1, 16, 11, 13, generator=g)
    with torch.no_grad():
        res['up_out'] = up(x, (40, 57))
    res['up_in'] = x
    res['up_size'] = np.array((40, 57))
    path = os.path.join(ROOT, 'tests', 'golden', 'g19_upsampler.npz')
    np.savez_compressed(path, **{k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in res.items()})
    print('g19_upsampler %.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
