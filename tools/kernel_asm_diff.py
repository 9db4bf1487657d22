"""Do two trees compile the per-frame kernels to the same gfx950 instructions?   python tools/kernel_asm_diff.py OLD_TREE NEW_TREE
Compiles refiner_ops.hip, target_model.hip and ragged_group.hip of both trees with build.py's flags plus -S --cuda-device-only and
compares, per kernel, the instruction lines: directives and comments dropped, .LBB labels renumbered in order of appearance.
One line per kernel, ``identical`` or the two instruction counts followed by the unified diff."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

FILES = {'refiner_ops.hip': ('k_tse_inject', 'k_cab_gate', 'k_cab_combine'), 'target_model.hip': ('k_track_merge',),
         'ragged_group.hip': ('k_tse_inject_indexed', 'k_cab_gate_indexed', 'k_cab_combine_indexed', 'k_track_merge_ragged')}
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function', '-S', '--cuda-device-only']      # build.py's


def kernels(tree, src, out):
    """{kernel name: its instruction lines} of one source file of one tree."""
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + FLAGS + [os.path.join(tree, 'frtm-vos_amd', 'csrc', src), '-o', out],
                          stderr=subprocess.DEVNULL)
    found, name = {}, None
    for ln in open(out):
        ln = ln.split(';')[0].rstrip()
        m = re.match(r'_Z(\d+)(\w+):$', ln)
        if m:                                                    # a mangled function label: _Z<length><name><argument types>
            name = m.group(2)[:int(m.group(1))]
            found[name] = []
        elif ln.startswith('.Lfunc_end'):
            name = None
        elif name and ln.strip() and (not ln.lstrip().startswith('.') or ln.startswith('.LBB')):
            found[name].append(ln.strip())
    for body in found.values():
        labels = {}
        for ln in body:
            for lab in re.findall(r'\.LBB\d+_\d+', ln):
                labels.setdefault(lab, '.L%d' % len(labels))
        body[:] = [re.sub(r'\.LBB\d+_\d+', lambda m: labels[m.group(0)], ln) for ln in body]
    return found


def main(old, new):
    with tempfile.TemporaryDirectory() as tmp:
        for src, names in FILES.items():
            a, b = kernels(old, src, os.path.join(tmp, 'old.s')), kernels(new, src, os.path.join(tmp, 'new.s'))
            for k in names:
                count = lambda body: sum(not ln.endswith(':') for ln in body)
                if a[k] == b[k]:
                    print('%-24s identical (%d instructions)' % (k, count(a[k])))
                else:
                    print('%-24s %d -> %d instructions' % (k, count(a[k]), count(b[k])))
                    print('\n'.join('    ' + ln for ln in difflib.unified_diff(a[k], b[k], 'old', 'new', lineterm='', n=2)))


if __name__ == '__main__':
    main(*sys.argv[1:3])
