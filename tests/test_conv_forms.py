"""The list of convolution kernel forms that tests/test_conv_forms_gpu.py must reach, and a check (no GPU needed) that it is complete: the four conv
translation units are compiled to gfx950 ISA and every kernel they define must be in FORMS or in EXCEPTIONS.  A kernel form added later without a case
in the GPU form matrix fails here.

Names are those frtm_conv_last_kernels() reports: the demangled symbol without spaces, namespace and argument list."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
SOURCES = ('conv_igemm.hip', 'conv_gemm32.hip', 'conv_wino.hip', 'conv_wino4.hip')

_IGEMM_TILES = ((128, 128, 2, 4), (128, 128, 4, 4), (128, 64, 2, 2), (32, 64, 1, 4), (64, 128, 2, 4), (64, 64, 2, 2), (64, 64, 2, 4))
FORMS = frozenset(
    ['k_conv_igemm<%d,%d,%d,%d,%d,32>' % (t + (mode,)) for t in _IGEMM_TILES for mode in (0, 1)]
    + ['k_conv_igemm<%d,%d,%d,%d,2,32>' % t for t in ((32, 64, 1, 4), (64, 64, 2, 2), (64, 64, 2, 4))]
    + ['k_conv3x3_halo<%d,%d,%d,%d,%d>' % (bm, wgm, wgn, tw, s)
       for bm, wgm, wgn in ((32, 1, 4), (64, 2, 2), (80, 1, 4), (128, 2, 2)) for tw in (4, 8, 16) for s in (1, 2)]
    + ['k_conv_igemm_p', 'k_splitk_epilogue', 'k_pack_weights', 'k_pack_weights_halo',
       'k_conv1x1_g32<1,1,2,2,0,2>',
       'k_conv3x3_wino<2,0,3>', 'k_conv3x3_wino<2,1,3>', 'k_conv3x3_wino<1,0,5>', 'k_pack_weights_wino',
       'k_wino4_weights', 'k_wino4_input', 'k_wino4_output', 'k_wino6_weights', 'k_wino6_input', 'k_wino6_output'])

# kernels that no call of the C ABI can launch: name -> reason (none today)
EXCEPTIONS = {}


def kernel_name(demangled):
    """'void k_conv_igemm<64, 64, 2, 2, 0, 32>(ConvParams)' -> 'k_conv_igemm<64,64,2,2,0,32>'."""
    s = demangled.replace('(anonymous namespace)::', '')
    s = re.sub(r'^void\s+', '', s)
    return s.split('(')[0].replace(' ', '')


def test_form_names():
    assert kernel_name('void (anonymous namespace)::k_conv1x1_g32<1, 1, 2, 2, 0, 2>(ConvParams)') == 'k_conv1x1_g32<1,1,2,2,0,2>'
    assert kernel_name('(anonymous namespace)::k_wino4_input(float const*, int, int)') == 'k_wino4_input'
    assert len(FORMS) == 56 - len(EXCEPTIONS)
    assert not FORMS & set(EXCEPTIONS)


def test_every_compiled_conv_kernel_is_a_listed_form():
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    filt = shutil.which('c++filt') or shutil.which('llvm-cxxfilt')
    assert filt, 'c++filt not found'
    with tempfile.TemporaryDirectory() as d:
        procs = []
        for src in SOURCES:
            out = os.path.join(d, src + '.s')
            procs.append((src, out, subprocess.Popen([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                                                      os.path.join(ROOT, 'frtm-vos_amd', 'csrc', src)],
                                                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=d)))
        mangled = []
        for src, out, p in procs:
            _, err = p.communicate()
            assert p.returncode == 0, (src, err.decode()[-2000:])
            mangled += re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', open(out).read(), flags=re.M)
    demangled = subprocess.run([filt], input='\n'.join(mangled), capture_output=True, text=True, check=True).stdout.split('\n')
    names = [kernel_name(n) for n in demangled if n.strip()]
    assert len(names) == len(mangled) == len(set(names)), names
    compiled = set(names)
    assert compiled - FORMS - set(EXCEPTIONS) == set(), 'kernel forms no test reaches: add cases to tests/test_conv_forms_gpu.py'
    assert (FORMS | set(EXCEPTIONS)) - compiled == set(), 'listed forms that no longer exist'
