"""oracle/make_golden_dropin.py -- TEST INFRASTRUCTURE ONLY; run in the build container:

    python oracle/make_golden_dropin.py      # writes tests/golden/g18_dropin.npz

Fixture G18: what the upstream driver (``evaluate.py``) hands the package when it is dropped onto it, recorded
so that tests/test_dropin_reference_driver.py needs nothing outside the repository:

  * ``imports``: every name the upstream ``evaluate.py`` imports from its ``model.*`` / ``lib.*`` modules, as [upstream module, name];
  * ``get_model_calls``: the call shape of the upstream ``Parameters.get_model()``, taken with ``ast`` in evaluation order: one row per call,
    [``'class'`` for a call of an imported name or ``'method'`` for an attribute call, callee name, number of positional arguments, keyword
    names] -- what the package's classes must accept for the upstream driver to build its pipeline on them;
  * ``params``: the upstream ``Parameters`` attributes (feature extractor, iteration schedules, augmentation / target-model / refiner
    hyper-parameters) for a ResNet-18 and a ResNet-101 checkpoint, full and fast schedule, and whether an unknown width is refused;
  * ``refiner_state``: the state dict layout of the UPSTREAM ``SegNetwork`` (ResNet-18 widths) as ``refiner.*`` checkpoint keys, in order,
    with shape and dtype of every tensor (the values are a seeded draw and carry no information: the test draws its own).
"""
import ast
import importlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = '/root/reference'
OUT = os.path.join(ROOT, 'tests', 'golden', 'g18_dropin.npz')
PKG_MODEL = ('tracker', 'discriminator', 'optimizer', 'memory', 'feature_extractor', 'seg_network', 'augmenter')
PKG_LIB = ('tensorlist', 'utils', 'image', 'datasets', 'evaluation')


class _EasyDict(dict):
    """Stand-in for easydict.EasyDict (absent here): attribute access, nested dicts converted."""

    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in dict(d or {}, **kw).items():
            self[k] = v

    def __setitem__(self, k, v):
        super().__setitem__(k, _EasyDict(v) if isinstance(v, dict) and not isinstance(v, _EasyDict) else v)

    __setattr__ = __setitem__

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def upstream_evaluate():
    import frtm_vos_amd  # noqa: F401
    ed = types.ModuleType('easydict')
    ed.EasyDict = _EasyDict
    sys.modules['easydict'] = ed
    sys.modules['model'] = importlib.import_module('frtm_vos_amd.model')
    sys.modules['lib'] = importlib.import_module('frtm_vos_amd.lib')
    for m in PKG_MODEL:
        sys.modules['model.' + m] = importlib.import_module('frtm_vos_amd.model.' + m)
    for m in PKG_LIB:
        sys.modules['lib.' + m] = importlib.import_module('frtm_vos_amd.lib.' + m)
    spec = importlib.util.spec_from_file_location('upstream_evaluate', os.path.join(REF, 'evaluate.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    for k in [k for k in sys.modules if k in ('model', 'lib') or k.startswith(('model.', 'lib.'))]:
        del sys.modules[k]
    return mod


def imports(tree):
    rows = []
    for node in tree.body:
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split('.')[0] in ('model', 'lib'):
            rows.extend([node.module, a.name] for a in node.names)
    return rows


def get_model_calls(tree, imported):
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'Parameters')
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == 'get_model')
    rows = []

    class Calls(ast.NodeVisitor):
        def visit_Call(self, node):              # post-order: receiver and arguments are evaluated before the call itself
            self.generic_visit(node)
            f = node.func
            if isinstance(f, ast.Name) and f.id in imported:
                rows.append(['class', f.id, len(node.args), [k.arg for k in node.keywords]])
            elif isinstance(f, ast.Attribute):
                rows.append(['method', f.attr, len(node.args), [k.arg for k in node.keywords]])
    Calls().visit(fn)
    return rows


def plain(v):
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v


def params(ev):
    rows = []
    for cin in (256, 1024):
        for fast in (False, True):
            p = ev.Parameters({'refiner.TSE.layer4.reduce.0.weight': torch.zeros(64, cin, 1, 1)}, fast=fast, device='cpu')
            rows.append(dict(in_channels=cin, fast=fast, feature_extractor=p.feature_extractor, init_iters=list(p.init_iters),
                             update_iters=list(p.update_iters), num_aug=p.num_aug, train_skipping=p.train_skipping,
                             learning_rate=p.learning_rate, aug_params=plain(p.aug_params), disc_params=plain(p.disc_params),
                             refnet_params=plain(p.refnet_params)))
    try:
        ev.Parameters({'refiner.TSE.layer4.reduce.0.weight': torch.zeros(64, 512, 1, 1)}, device='cpu')
        refused = None
    except Exception as ex:      # noqa: BLE001
        refused = type(ex).__name__
    return dict(cases=rows, unknown_width_512_raises=refused)


def upstream_refiner_state(in_channels):
    """State dict of the UPSTREAM SegNetwork (model/seg_network.py, pure torch), as 'refiner.*' checkpoint keys."""
    spec = importlib.util.spec_from_file_location('upstream_seg_network', os.path.join(REF, 'model', 'seg_network.py'))
    mod = importlib.util.module_from_spec(spec)
    lib = types.ModuleType('lib')
    lib_utils = types.ModuleType('lib.utils')
    ref_utils = importlib.util.spec_from_file_location('upstream_lib_utils', os.path.join(REF, 'lib', 'utils.py'))
    um = importlib.util.module_from_spec(ref_utils)
    ref_utils.loader.exec_module(um)
    lib_utils.__dict__.update({k: v for k, v in um.__dict__.items() if not k.startswith('__')})
    lib.utils = lib_utils
    sys.modules['lib'], sys.modules['lib.utils'] = lib, lib_utils
    try:
        spec.loader.exec_module(mod)
    finally:
        del sys.modules['lib'], sys.modules['lib.utils']
    from collections import OrderedDict
    chans = OrderedDict(layer5=in_channels * 2, layer4=in_channels, layer3=in_channels // 2, layer2=in_channels // 4)
    torch.manual_seed(5)
    net = mod.SegNetwork(1, 64, chans, True)
    return {'refiner.' + k: v.clone() for k, v in net.state_dict().items()}


def main():
    ev = upstream_evaluate()
    tree = ast.parse(open(os.path.join(REF, 'evaluate.py')).read())
    imp = imports(tree)
    for module, name in imp:                     # (every imported name was bound by the execution above)
        assert getattr(ev, name).__module__.startswith('frtm_vos_amd.'), (module, name)
    out = {'imports': np.array(json.dumps(imp)), 'params': np.array(json.dumps(params(ev))),
           'get_model_calls': np.array(json.dumps(get_model_calls(tree, {n for _, n in imp})))}
    state = upstream_refiner_state(256)
    out['refiner_state'] = np.array(json.dumps([[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in state.items()]))
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, '%.0f KB' % (os.path.getsize(OUT) / 1024))


if __name__ == '__main__':
    main()
