"""Do the kernels of the working tree compile to the same gfx950 machine code as those of a git revision?

For every `.hip` file of `build.SOURCES` the revision's copy and the working tree's copy are compiled with `build.FLAGS` plus
`-S --cuda-device-only`, the lines that hold `__hip_cuid_` are dropped (that symbol is a hash of the source text: it changes when a
comment moves) and the two listings are compared byte for byte.  Whole listings only: no instruction is looked at.  Needs hipcc, no GPU.

    python tools/listing_diff.py [--rev HEAD] [--jobs 8] [--work DIR] [--out profiles/rNN_listing_diff.txt] [file.hip ...]

One line per translation unit: line count and sha256 of the filtered listing on both sides.  Exit status 1 if any pair differs.
`--work DIR` keeps the listings there (and reuses the revision's listings of an earlier call for the same commit).
"""
import argparse
import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'sc2-benchmark_amd'


def load_build():
    spec = importlib.util.spec_from_file_location('sc2_build', os.path.join(ROOT, PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def listing(build, tree, src, out):
    """Compiles tree/PKG/csrc/src to the listing `out` (from inside csrc, so that both sides name their files alike)."""
    if not os.path.exists(out):
        cmd = [build.HIPCC] + build.FLAGS + ['-x', 'hip', '-S', '--cuda-device-only', src, '-o', out + '.tmp']
        subprocess.check_call(cmd, cwd=os.path.join(tree, PKG, 'csrc'))
        os.replace(out + '.tmp', out)
    lines = [l for l in open(out, 'rb') if b'__hip_cuid_' not in l]
    return len(lines), hashlib.sha256(b''.join(lines)).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rev', default='HEAD')
    ap.add_argument('--jobs', type=int, default=8)
    ap.add_argument('--work', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('files', nargs='*')
    a = ap.parse_args()
    build = load_build()
    sha = subprocess.check_output(['git', 'rev-parse', a.rev], cwd=ROOT, text=True).strip()
    work = a.work or tempfile.mkdtemp(prefix='listing_diff_')
    base_tree, base_s, head_s = (os.path.join(work, d) for d in ('tree_' + sha[:12], 'base_' + sha[:12], 'tree'))
    for d in (base_tree, base_s, head_s):
        os.makedirs(d, exist_ok=True)
    archive = subprocess.Popen(['git', 'archive', sha, PKG + '/csrc', 'include'], cwd=ROOT, stdout=subprocess.PIPE)
    subprocess.check_call(['tar', '-x', '-C', base_tree], stdin=archive.stdout)
    if archive.wait():
        sys.exit('git archive failed')
    for f in os.listdir(head_s):                       # the working tree is compiled afresh on every call
        os.remove(os.path.join(head_s, f))
    srcs = a.files or [s for s in build.SOURCES if s.endswith('.hip')]

    def one(src):
        b = listing(build, base_tree, src, os.path.join(base_s, src + '.s'))
        h = listing(build, ROOT, src, os.path.join(head_s, src + '.s'))
        return src, b, h

    with ThreadPoolExecutor(max_workers=a.jobs) as ex:
        rows = list(ex.map(one, srcs))
    text = ['# filtered listings (lines with __hip_cuid_ dropped) of %s (%s) against the working tree' % (a.rev, sha[:12]),
            '# translation unit | lines, sha256 at the revision | lines, sha256 in the tree | verdict']
    bad = 0
    for src, b, h in rows:
        same = b == h
        bad += not same
        text.append('%-22s %7d %s  %7d %s  %s' % (src, b[0], b[1], h[0], h[1], 'identical' if same else 'DIFFERENT'))
    text.append('# %d translation units, %d identical, %d different' % (len(rows), len(rows) - bad, bad))
    print('\n'.join(text))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
