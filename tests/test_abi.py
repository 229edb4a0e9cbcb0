"""The C-ABI library loads, exports every symbol include/sc2_bottleneck.h declares, and its HOST function
(CDF quantisation) is bit-exact against the oracle.  No device compute here."""
import os
import re

import numpy as np
import pytest

from oracle import rans as oracle_rans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'sc2_bottleneck.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(sc2_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_declared_symbol(S):
    lib = S.hip.lib()
    declared = _declared_symbols()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), 'libsc2amd.so does not export {}'.format(name)
    assert sorted(S.hip.ABI_SYMBOLS) == declared
    assert lib.sc2_abi_version() == 51


def test_missing_library_fails_loudly(S, monkeypatch):
    monkeypatch.setattr(S.hip, '_lib', None)
    monkeypatch.setattr(S.hip, 'LIB_PATH', '/nonexistent/libsc2amd.so')
    with pytest.raises(S.hip.Sc2Error, match='no CPU fallback'):
        S.hip.lib()


def test_cpu_tensor_is_rejected(S):
    import torch
    with pytest.raises(S.hip.Sc2Error, match='no CPU fallback'):
        S.hip.nchw_f32_to_nhwc_bf16(torch.zeros(1, 3, 4, 4))
    m = S.FPBasedResNetBottleneck()
    with torch.no_grad(), pytest.raises(S.hip.Sc2Error):
        m(torch.zeros(1, 3, 32, 32))


def test_host_cdf_matches_oracle(S):
    rng = np.random.RandomState(1)
    for n in (1, 2, 5, 23, 64, 257):
        for power in (1, 3, 8):
            p = rng.rand(n).astype(np.float32) ** power
            p /= max(p.sum(), 1e-30)
            got = S.hip.pmf_to_quantized_cdf(p.tolist())
            want = oracle_rans.pmf_to_quantized_cdf(p)
            assert got.tolist() == [int(v) for v in want]
    assert S.hip.pmf_to_quantized_cdf([1e-9, 0.5, 0.5 - 2e-9, 1e-9]).tolist() == [0, 1, 32767, 65535, 65536]
    with pytest.raises(ValueError):
        S.hip.pmf_to_quantized_cdf([0.3, -0.2])
    with pytest.raises(ValueError):
        S.hip.pmf_to_quantized_cdf([0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        S.hip.pmf_to_quantized_cdf([float('nan'), 0.5])


def test_sizing_helpers(S):
    lib = S.hip.lib()
    assert [lib.sc2_conv_weight_rows(c) for c in (24, 48, 64, 96, 256, 512, 1000)] == [32, 48, 64, 96, 256, 512, 1024]
    assert [lib.sc2_conv_weight_pitch(k) for k in (75, 96, 120, 2400)] == [128, 128, 128, 2432]
    assert S.hip.rans_max_bytes(0) >= 8 and S.hip.rans_max_bytes(72600) >= 72600 * 52 // 8


def test_raw_claim_atomics_are_read_behind_their_wait():
    """The persistent kernels claim work with a raw `global_atomic_add` whose destination register hipcc believes is
    written at the asm statement; if the compiler copies or spills it before the counted wait, claims go stale and the
    unit loop never ends (seen once).  tools/audit_asm_atomic.py compiles the kernels to ISA and checks the first
    reader of every such register."""
    import os
    import subprocess
    import sys
    if not os.path.exists('/opt/rocm/bin/hipcc'):
        import pytest
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'audit_asm_atomic.py')], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count('ok ') >= 14 and 'BAD' not in r.stdout, r.stdout


def test_asm_weight_loads_are_never_copied_in_flight():
    """The window-plane kernels and the fused decoder head load their weight fragments by inline asm and wait for them
    with hand-counted `s_waitcnt vmcnt(N)` (the compiler's scoreboard turned the prefetch into a drain of freshly issued
    window pieces).  What the compiler does not know is that such a register is valid only behind its wait: a copy or
    a spill placed between the load and the wait reads stale data (seen: a tied wait operand made hipcc copy the
    fragment IN FRONT of the wait; the forward-GDN1 variant spilled fragments across its epilogue).
    tools/audit_vmcnt.py --copies compiles the kernels to ISA and follows every marked load (`; wfrag`) through the
    control-flow graph to its first MFMA: nothing else may read the register on the way.  The loads, the waits and the rules
    they are written to are in csrc/gfx950_prims.h."""
    import os
    import subprocess
    import sys
    if not os.path.exists('/opt/rocm/bin/hipcc'):
        import pytest
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, 'sc2-benchmark_amd', 'csrc')
    files = [os.path.join(csrc, f) for f in ('conv2x2_win.hip', 'conv3x3_win.hip', 'conv1x1_win.hip', 'conv_gdn512.hip', 'conv2_gdn48.hip', 'conv_f32.hip', 'gdn512_rows.hip')]
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'audit_vmcnt.py'), '--copies'] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # the second hazard the compiler does not cover: a 16-byte buffer store with an SGPR soffset directly followed by a VALU write
    # of its data registers (tools/micro/store_hazard.hip; buf_store16 of csrc/gfx950_prims.h carries the wait states)
    stores = [os.path.join(csrc, f) for f in ('conv2x2_win.hip', 'conv1x1_pair.hip', 'conv3x3_win.hip', 'conv1x1_win.hip', 'gdn512_rows.hip')]
    r2 = subprocess.run([sys.executable, os.path.join(root, 'tools', 'audit_vmcnt.py'), '--stores'] + stores, capture_output=True, text=True)
    assert r2.returncode == 0 and r2.stdout.count(': ok') == len(stores), r2.stdout + r2.stderr
    assert r.stdout.count(': ok') == len(files) and 'COPY?' not in r.stdout, r.stdout
    # round 5, the third check: is every counted wait SMALL enough?  `--counts` follows each register an inline-asm load (or returning
    # atomic) writes through the control-flow graph with the number of vector-memory operations issued behind it (the model the
    # kernels are written to: in-order retirement); a `vmcnt(N)` with a larger N does not wait for it -- the class of commit 9bc486e
    # (conv0_gdn_f32_persist's first tile), which --copies cannot see.  Every file with hand-written vector-memory asm goes through
    # it EXCEPT conv2x2_win.hip: there a wave-uniform runtime condition selects both how many window fills a k-step issues and which
    # wait constant it uses (correlated branches), which a path-insensitive analysis cannot pair up -- that kernel stays under
    # --copies and its bit-identity tests (tests/test_gpu_kernels.py::test_conv2x2_win*).
    counted = [os.path.join(csrc, f) for f in ('conv0_gdn96.hip', 'conv1x1_kres.hip', 'conv1x1_pair.hip', 'conv1x1_stream.hip', 'conv1x1_win.hip',
                                               'conv2_gdn48.hip', 'conv3x3_win.hip', 'conv_gdn512.hip', 'conv_f32.hip', 'conv_dec_persist.hip',
                                               'conv_wgrad.hip', 'rans.hip', 'conv_inst_a.hip', 'conv_inst_c.hip', 'conv_inst_e.hip', 'gdn512_rows.hip')]
    from concurrent.futures import ThreadPoolExecutor     # (one hipcc -S per file: six at a time)
    tool = os.path.join(root, 'tools', 'audit_vmcnt.py')
    with ThreadPoolExecutor(max_workers=6) as ex:
        runs = list(ex.map(lambda f: subprocess.run([sys.executable, tool, '--counts', f], capture_output=True, text=True), counted))
    for f, r3 in zip(counted, runs):
        assert r3.returncode == 0 and ': ok' in r3.stdout and 'COUNT?' not in r3.stdout, f + '\n' + r3.stdout + r3.stderr
    # the fourth (round 5): no compiler spill / copy of a register that ANY inline-asm load (fragments, the backward's per-lane gradient
    # loads) is still filling, by the same in-order model -- tools/audit_inflight.py on the listing of the kernel that showed the case
    # (gdn512_rows.hip: two of twelve ring registers spilled right behind their loads, GEMM 2 ran on stale registers)
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        lst = os.path.join(td, 'rows.s')
        subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-D__HIP_PLATFORM_AMD__=1', '-x', 'hip',
                               '--cuda-device-only', '-S', os.path.join(csrc, 'gdn512_rows.hip'), '-o', lst], stderr=subprocess.DEVNULL)
        r4 = subprocess.run([sys.executable, os.path.join(root, 'tools', 'audit_inflight.py'), lst], capture_output=True, text=True)
    assert r4.returncode == 0 and '0 finding(s)' in r4.stdout, r4.stdout + r4.stderr
    # the fifth (round 5): conv_wgrad.hip reads a slab's fragments from LDS by asm one slab AHEAD of its MFMAs; the wait is the
    # `lgkmcnt(0)` of the next step -- nothing may read, copy or overwrite those registers on the way (tools/audit_lds_inflight.py)
    r5 = subprocess.run([sys.executable, os.path.join(root, 'tools', 'audit_lds_inflight.py'), os.path.join(csrc, 'conv_wgrad.hip')],
                        capture_output=True, text=True)
    assert r5.returncode == 0 and '6 kernel(s)' in r5.stdout and ' 0 finding(s)' in r5.stdout, r5.stdout + r5.stderr


def test_hot_path_kernels_use_no_scratch():
    """Read from the built library's code objects (tools/kernel_resources.py): no kernel of the default path may spill
    to scratch.  (A shared-header edit once demoted the 256-wide decoder kernels' accumulators to 528 B / lane of
    scratch: +20 % on dec.conv2 with every parity test green.)  Known exceptions: the opt-in experiment kernels."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('kernel_resources', os.path.join(root, 'tools', 'kernel_resources.py'))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(os.path.join(root, 'sc2-benchmark_amd', 'libsc2amd.so'))
    assert len(ks) > 60
    opt_in = ('conv_igemm4_kernel',                   # SC2_CONV_BIG4 experiment (4-wave register tile)
              'ELi128ELi3ELb0ELi64EEEEEvNS_8ConvArgsE',   # SC2_CONV_HALF experiment (128-row tile, 128-register cap)
              # the training-step GDN1 kernels (round 5) sit at the 256-register cap of two waves per SIMD: 9 - 31 dwords of loop
              # invariants and one accumulator tile go to scratch (36 - 124 B / lane; measured with them: 512-channel backward
              # 2.45 -> 1.22 ms).  What may NOT happen there -- a spill of a register an asm load is still filling -- is checked by
              # tools/audit_inflight.py and audit_vmcnt.py --copies (test above).
              'gdn512_rows_kernelILi512E', 'gdn96_strips_kernelILi1E',
              # the t-emitting (training) instantiations of the fused first decoder stage: 96 - 144 B / lane of tile-loop invariants
              # (patch / slot addresses), written once in the prologue and read back in the epilogue -- none inside phase 2
              'ELb1EEEvNS_7DecArgsE')
    bad = [(k['name'], k['scratch']) for k in ks if k['scratch'] and not any(o in k['name'] for o in opt_in)]
    assert not bad, 'kernels with scratch: {}'.format(bad)
    big = [k for k in ks if 'conv_igemm8_kernel' in k['name'] and 'ELi256ELi4ELb0ELi64' in k['name']]
    assert big and all(k['vgpr'] <= 256 for k in big)          # two waves per SIMD (the two-group schedule)
