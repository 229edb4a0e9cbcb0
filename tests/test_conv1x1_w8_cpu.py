"""The eight-wave 256-channel 1x1 kernel (conv1x1_w8.hip) without a GPU: register budget of the built code objects and the listing
audits of its hand-counted waits, called the way tests/test_abi.py calls them for the other hand-counted kernels."""
import importlib.util
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'sc2-benchmark_amd', 'csrc', 'conv1x1_w8.hip')
HIPCC = '/opt/rocm/bin/hipcc'


def test_no_scratch_and_two_waves_per_simd():
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(ROOT, 'tools', 'kernel_resources.py'))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = [k for k in kr.kernels(os.path.join(ROOT, 'sc2-benchmark_amd', 'libsc2amd.so')) if 'conv1x1_w8_kernel' in k['name']]
    assert len(ks) == 4, [k['name'] for k in ks]          # relu x residual
    for k in ks:
        assert k['scratch'] == 0 and k['spill_vgpr'] == 0, k
        assert k['vgpr'] + k['agpr'] <= 256, k            # 512 threads = two waves per SIMD


def test_listing_audits():
    """--counts: every counted wait is small enough on every path (one instruction stream for first and later units);
    --copies: nothing but an MFMA reads a fragment register in flight;  --stores: every 16-byte store carries its wait states;
    audit_inflight: no spill or copy of a register an asm load is filling.  No raw atomics: units are claimed by a static interleave."""
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    tool = os.path.join(ROOT, 'tools', 'audit_vmcnt.py')
    for mode in ('--counts', '--copies', '--stores'):
        r = subprocess.run([sys.executable, tool, mode, SRC], capture_output=True, text=True)
        assert r.returncode == 0 and 'conv1x1_w8.hip: ok' in r.stdout, mode + '\n' + r.stdout + r.stderr
        assert 'COUNT?' not in r.stdout and 'COPY?' not in r.stdout and 'STORE?' not in r.stdout, r.stdout
    with tempfile.TemporaryDirectory() as td:
        lst = os.path.join(td, 'w8.s')
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-D__HIP_PLATFORM_AMD__=1', '-x', 'hip',
                               '--cuda-device-only', '-S', SRC, '-o', lst], stderr=subprocess.DEVNULL)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'audit_inflight.py'), lst], capture_output=True, text=True)
        text = open(lst).read()
    assert r.returncode == 0 and '0 finding(s)' in r.stdout, r.stdout + r.stderr
    assert text.count('; wfrag') >= 4 * 24 and 'global_atomic' not in text
