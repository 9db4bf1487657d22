"""The upstream driver really drops onto the package (north_star: "the reference evaluate.py drops onto it unchanged").

Fixture G18 (oracle/make_golden_dropin.py) records, from the upstream ``evaluate.py`` run under INTEGRATION.md section A's aliasing (the
package's module tree under the upstream names ``model`` / ``lib``): the names it imports, the call shape of its ``Parameters.get_model()``
(callee, number of positional arguments, keyword names of every call, in evaluation order), the hyper-parameters of its ``Parameters`` for
a ResNet-18 and a ResNet-101 checkpoint (full and fast schedule), and the layout of the UPSTREAM ``SegNetwork``'s state dict (``refiner.*``
checkpoint keys, shapes, dtypes).  Here the aliasing is applied again: every recorded import must resolve to the package's object,
upstream's ``get_model()`` is replayed on the package's classes in exactly the recorded call shape and must build the package's
``Tracker`` from an upstream-shaped checkpoint, the upstream hyper-parameters must arrive in the package's ``Discriminator``, and
``load_state_dict`` must accept exactly the upstream keys.  No GPU here: the extractor's upload to the device is stubbed, nothing is computed.
"""
import importlib
import inspect
import json
import sys

import pytest
import torch

PKG_MODEL = ('tracker', 'discriminator', 'optimizer', 'memory', 'feature_extractor', 'seg_network', 'augmenter')
PKG_LIB = ('tensorlist', 'utils', 'image', 'datasets', 'evaluation')


@pytest.fixture
def g18(golden):
    z = golden('g18_dropin')
    return {k: json.loads(str(z[k])) for k in z.files}


@pytest.fixture
def aliased():
    """the package's module tree under the upstream names."""
    import frtm_vos_amd  # noqa: F401
    saved = {k: v for k, v in sys.modules.items() if k in ('model', 'lib') or k.startswith(('model.', 'lib.'))}
    for k in saved:
        del sys.modules[k]
    sys.modules['model'] = importlib.import_module('frtm_vos_amd.model')
    sys.modules['lib'] = importlib.import_module('frtm_vos_amd.lib')
    for m in PKG_MODEL:
        sys.modules['model.' + m] = importlib.import_module('frtm_vos_amd.model.' + m)
    for m in PKG_LIB:
        sys.modules['lib.' + m] = importlib.import_module('frtm_vos_amd.lib.' + m)
    try:
        yield
    finally:
        for k in [k for k in sys.modules if k in ('model', 'lib') or k.startswith(('model.', 'lib.'))]:
            del sys.modules[k]
        sys.modules.update(saved)


def _upstream_refiner_state(g18):
    """An upstream-shaped checkpoint: the UPSTREAM SegNetwork's 'refiner.*' keys, shapes and dtypes (G18), seeded values."""
    gen = torch.Generator().manual_seed(5)
    out = {}
    for k, shape, dtype in g18['refiner_state']:
        dt = getattr(torch, dtype)
        out[k] = torch.randn(shape, generator=gen).to(dt) if dt.is_floating_point else torch.randint(0, 9, shape, generator=gen).to(dt)
    return out


def _upstream_case(g18, in_channels, fast):
    return next(c for c in g18['params']['cases'] if c['in_channels'] == in_channels and c['fast'] == fast)


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def test_upstream_evaluate_drops_onto_the_package(g18, aliased, monkeypatch):
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.model import augmenter, discriminator, feature_extractor, seg_network, tracker
    from frtm_vos_amd.lib import datasets, evaluation
    # (1) every name the upstream driver imports (evaluate.py:18-23) resolves, under the aliasing, to the package's object
    got = {name: getattr(importlib.import_module(module), name) for module, name in g18['imports']}
    assert len(got) == len(g18['imports']) == 7
    assert got['Tracker'] is tracker.Tracker
    assert got['ResnetFeatureExtractor'] is feature_extractor.ResnetFeatureExtractor
    assert got['SegNetwork'] is seg_network.SegNetwork
    assert got['ImageAugmenter'] is augmenter.ImageAugmenter
    assert got['DAVISDataset'] is datasets.DAVISDataset and got['YouTubeVOSDataset'] is datasets.YouTubeVOSDataset
    assert got['evaluate_dataset'] is evaluation.evaluate_dataset
    # (2) an upstream-shaped checkpoint (ResNet-18 variant: autodetected from the refiner's layer4 reduce conv, :38-44), read like upstream reads it
    weights = _upstream_refiner_state(g18)
    assert weights['refiner.TSE.layer4.reduce.0.weight'].shape[1] == 256
    up = _upstream_case(g18, 256, False)
    assert up['feature_extractor'] == 'resnet18' and up['init_iters'] == [5, 10, 10, 10, 10] and up['update_iters'] == [10]
    assert _upstream_case(g18, 256, True)['init_iters'] == [5, 10, 10, 10]
    p = Parameters(weights, device='cpu')
    assert p.feature_extractor == up['feature_extractor'] and list(p.init_iters) == up['init_iters'] and list(p.update_iters) == up['update_iters']
    assert list(Parameters(weights, fast=True, device='cpu').init_iters) == _upstream_case(g18, 256, True)['init_iters']
    # (3) upstream's get_model() (evaluate.py:91-105) replayed on the package's classes in its recorded call shape (G18 get_model_calls):
    # every constructor call goes to the class the upstream name resolves to, with exactly the recorded number of positional arguments and
    # keyword names, so that a keyword the package made required or a changed positional order fails here.  The values are the upstream
    # hyper-parameters (equal to the package's Parameters: test_upstream_parameters_match_the_packages_own_driver).
    dev = 'cuda:0' if torch.cuda.is_available() else 'cpu'
    if dev == 'cpu':                                                           # no GPU here: the extractor's device upload is stubbed
        monkeypatch.setattr(feature_extractor.ResnetFeatureExtractor, 'to', lambda self, device: self)
    p = Parameters(weights, device=dev)
    calls = g18['get_model_calls']
    shape = {name: (npos, kws) for kind, name, npos, kws in calls if kind == 'class'}
    assert list(shape) == ['ImageAugmenter', 'ResnetFeatureExtractor', 'SegNetwork', 'Tracker']          # construction order
    assert [kind for kind, *_ in calls].count('class') == len(shape)                                     # each class built once

    def make(name, *args):
        npos, kws = shape[name]
        assert len(args) == npos and kws == [], (name, npos, kws)             # upstream's positional arguments, no keywords
        return got[name](*args)

    aug = make('ImageAugmenter', p.aug_params)
    ext = make('ResnetFeatureExtractor', p.feature_extractor).to(dev)
    p.disc_params.in_channels = ext.get_out_channels()[p.disc_params.layer]
    outs = ext.get_out_channels()
    chans = {L: n for L, n in outs.items() if L in p.refnet_params.layers}
    refiner = make('SegNetwork', p.disc_params.out_channels, p.refnet_params.nchannels, chans, p.refnet_params.use_batch_norm)
    mdl = make('Tracker', aug, ext, p.disc_params, refiner, dev)
    mdl.load_state_dict(weights)
    mdl.to(dev)

    def accepts(obj, method, npos, kws):
        m = getattr(obj, method, None)
        if not callable(m):
            return False
        try:
            inspect.signature(m).bind(*([None] * npos), **{k: None for k in kws})
        except TypeError:
            return False
        except ValueError:                                                     # (a builtin without a signature)
            return True
        return True
    for kind, name, npos, kws in calls:                # every method call upstream makes is accepted, in its recorded shape, by the replay's objects
        if kind == 'method':
            assert any(accepts(o, name, npos, kws) for o in (ext, outs, mdl)), (name, npos, kws)
    assert type(mdl) is tracker.Tracker and type(mdl.refiner) is seg_network.SegNetwork
    assert type(mdl.feature_extractor) is feature_extractor.ResnetFeatureExtractor and mdl.feature_extractor.name == 'resnet18'
    assert p.disc_params.in_channels == 256                                    # read back from get_out_channels() (:95)
    for k, v in weights.items():                                               # the checkpoint really arrived in the refiner
        assert torch.equal(mdl.state_dict()[k].cpu(), v), k
    assert set(mdl.state_dict().keys()) == set(weights.keys())                 # "exactly the refiner.* keys" 
    own = Parameters(weights, device=dev).get_model()                          # the package's own driver builds the same model
    assert type(own) is tracker.Tracker and own.state_dict().keys() == mdl.state_dict().keys()
    assert all(torch.equal(own.state_dict()[k].cpu(), v) for k, v in weights.items())
    # (4) the upstream hyper-parameters arrive in the package's Discriminator through TargetObject(disc_params=...) (tracker.py:21-22)
    t = tracker.TargetObject(obj_id=1, disc_params=mdl.disc_params, index=1, start_frame=0, start_mask=None)
    d = t.discriminator
    assert type(d) is discriminator.Discriminator and t.disc_layer == 'layer4'
    assert d.project.weight.shape == (96, 256, 1, 1) and d.filter.weight.shape == (1, 96, 3, 3)
    assert d.init_iters == (5, 10, 10, 10, 10) and d.update_iters == (10,) and d.memory_size == 80 and d.train_skipping == 8
    assert d.filter_reg == (1e-4, 1e-2) and d.precond == (1e-4, 1e-2) and d.learning_rate == 0.1 and d.update_filters is True
    assert d.pw_params == dict(method='hinge', tf=0.1)
    assert abs(d.direction_forget_factor - 0.9 ** 750) < 1e-40
    # (5) strictness: a checkpoint with a missing or a foreign key is refused like upstream's nn.Module would
    bad = dict(weights)
    bad.pop('refiner.TSE.layer4.reduce.0.weight')
    with pytest.raises(RuntimeError):
        mdl.load_state_dict(bad)
    with pytest.raises(RuntimeError):
        mdl.load_state_dict(dict(weights, **{'feature_extractor.conv1.weight': torch.zeros(1)}))


def test_upstream_parameters_match_the_packages_own_driver(g18):
    """The package's evaluate.Parameters (its own driver) carries the same hyper-parameters as upstream's (evaluate.py:32-34,46-89), for both
    checkpoint widths and both schedules, and refuses a width upstream refuses."""
    from frtm_vos_amd.evaluate import Parameters as Own
    assert [c['feature_extractor'] for c in g18['params']['cases'] if c['in_channels'] == 1024] == ['resnet101', 'resnet101']
    for up in g18['params']['cases']:
        own = Own({'refiner.TSE.layer4.reduce.0.weight': torch.zeros(64, up['in_channels'], 1, 1)}, fast=up['fast'], device='cpu')
        assert own.feature_extractor == up['feature_extractor']
        assert list(own.init_iters) == up['init_iters'] and list(own.update_iters) == up['update_iters']
        assert (own.num_aug, own.train_skipping, own.learning_rate) == (up['num_aug'], up['train_skipping'], up['learning_rate'])
        assert set(up['disc_params']) <= set(own.disc_params)
        assert up['disc_params'] == {k: v for k, v in _plain(dict(own.disc_params)).items() if k in up['disc_params']}
        assert up['refnet_params'] == _plain(own.refnet_params)
        assert up['aug_params'] == _plain(own.aug_params)
    assert g18['params']['unknown_width_512_raises'] == 'ValueError'
    with pytest.raises(ValueError):
        Own({'refiner.TSE.layer4.reduce.0.weight': torch.zeros(64, 512, 1, 1)}, device='cpu')
