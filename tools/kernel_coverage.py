"""Which kernels of the built library does the GPU suite launch?  Joins two lists:

  * the kernels in libsc2amd.so, read from its gfx950 code objects the way tools/kernel_resources.py reads them;
  * the kernels a test run launched: the `*kernel_stats.csv` files of `rocprofv3 --kernel-trace --stats -- python -m pytest ...`
    (tracing only, no counters; one file per traced process -- give a directory and every file under it is summed).

    # on the GPU box, two runs (the test_00_* files start child benchmarks and are left out):
    rocprofv3 --kernel-trace --stats --output-format csv -d cov/base -- python -m pytest tests -q -m gpu \
        --ignore=tests/test_gpu_exact_conv.py --ignore=tests/test_00_bench_plain_gpu.py --ignore=tests/test_00_rccl_gpu.py
    rocprofv3 --kernel-trace --stats --output-format csv -d cov/exact -- python -m pytest tests/test_gpu_exact_conv.py -q -m gpu
    python tools/kernel_coverage.py --base cov/base --new cov/exact [--lib path/to/lib.so] [-o profiles/<name>.txt]

One line per library kernel: launches in the base run, launches in the new run, or "never" (in neither).  Launched kernels that are
not in the library (torch's own) are counted at the end, not listed.  A tool and a record: nothing in the suite calls it."""
import argparse
import csv
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def demangle(names):
    """Mangled names -> demangled, through c++filt (binutils) or llvm-cxxfilt (ROCm); names it does not know come back as they are."""
    for tool in ('c++filt', '/opt/rocm/llvm/bin/llvm-cxxfilt', 'llvm-cxxfilt'):
        try:
            out = subprocess.run([tool], input='\n'.join(names) + '\n', capture_output=True, text=True, check=True).stdout
        except (OSError, subprocess.CalledProcessError):
            continue
        lines = out.split('\n')[:len(names)]
        if len(lines) == len(names):
            return lines
    raise RuntimeError('no C++ demangler found (c++filt / llvm-cxxfilt)')


def key(name):
    """One spelling for a kernel name whoever demangled it: no return type, no '.kd', no argument list, no spaces, one spelling
    of the integer-literal suffixes and of bool template arguments."""
    s = name.strip().strip('"')
    if s.endswith('.kd'):
        s = s[:-3]
    s = re.sub(r'\s*\[clone [^\]]*\]', '', s)
    if s.startswith('void '):
        s = s[5:]
    depth, cut = 0, len(s)
    for i in range(len(s) - 1, -1, -1):      # drop the trailing (argument list)
        c = s[i]
        if c == ')':
            depth += 1
        elif c == '(':
            depth -= 1
            if depth == 0:
                cut = i
                break
    if s.endswith(')'):
        s = s[:cut]
    s = s.replace(' ', '')
    s = re.sub(r'\((?:int|unsigned|unsignedint|long|bool)\)', '', s)      # "(int)3" -> "3"
    s = re.sub(r'(?<=[<,])(\d+)(?:u|l|ul|ll|ull)(?=[,>])', r'\1', s)
    return s


def read_stats(path):
    """{key: calls} summed over every *kernel_stats.csv under `path` (a file or a directory)."""
    files = []
    if os.path.isdir(path):
        for d, _, fs in os.walk(path):
            files += [os.path.join(d, f) for f in fs if f.endswith('kernel_stats.csv')]
    else:
        files = [path]
    calls = {}
    for f in sorted(files):
        with open(f, newline='') as fh:
            for row in csv.DictReader(fh):
                k = key(row['Name'])
                calls[k] = calls.get(k, 0) + int(row['Calls'])
    return calls, files


def library_kernels(lib):
    mangled = sorted({k['name'] for k in kernel_resources.kernels(lib)})
    return list(zip(mangled, demangle(mangled)))


def table(lib, base, new):
    rows, seen = [], set()
    for mangled, dem in library_kernels(lib):
        k = key(dem)
        seen.add(k)
        rows.append((dem if dem != mangled else mangled, base.get(k, 0), new.get(k, 0)))
    foreign_base = sum(1 for k in base if k not in seen)
    foreign_new = sum(1 for k in new if k not in seen)
    return rows, foreign_base, foreign_new


def short(dem):
    s = dem.strip()
    if s.startswith('void '):
        s = s[5:]
    s = s.replace('(anonymous namespace)::', '').replace('sc2conv::', '')
    depth = 0
    for i in range(len(s) - 1, -1, -1):
        if s[i] == ')':
            depth += 1
        elif s[i] == '(':
            depth -= 1
            if depth == 0:
                return s[:i]
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--lib', default=os.path.join(ROOT, 'sc2-benchmark_amd', 'libsc2amd.so'))
    ap.add_argument('--base', required=True, help="kernel_stats.csv (or a directory of them) of the suite without the new file")
    ap.add_argument('--new', required=True, help='... of the new test file alone')
    ap.add_argument('-o', '--output')
    a = ap.parse_args()
    base, bf = read_stats(a.base)
    new, nf = read_stats(a.new)
    rows, fb, fn = table(a.lib, base, new)
    out = ['# kernels of {} against two traced test runs ({} + {} stats files)'.format(os.path.basename(a.lib), len(bf), len(nf)),
           '# {:>9} {:>9}  kernel'.format('base', 'new')]
    never = 0
    for name, b, n in sorted(rows, key=lambda r: short(r[0])):
        if not b and not n:
            never += 1
            out.append('  {:>9} {:>9}  {}'.format('never', 'never', short(name)))
        else:
            out.append('  {:>9} {:>9}  {}'.format(b or '-', n or '-', short(name)))
    only_new = sum(1 for _, b, n in rows if n and not b)
    out.append('# {} library kernels: {} launched by the base run, {} by the new run ({} of them by it alone), {} never'.format(
        len(rows), sum(1 for _, b, _ in rows if b), sum(1 for _, _, n in rows if n), only_new, never))
    out.append('# kernels launched that are not in the library (torch, rocBLAS, ...): {} names in the base run, {} in the new run'.format(fb, fn))
    text = '\n'.join(out) + '\n'
    if a.output:
        with open(a.output, 'w') as fh:
            fh.write(text)
    sys.stdout.write(text)


if __name__ == '__main__':
    main()
