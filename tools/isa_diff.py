#!/usr/bin/env python3
"""Does a refactor leave a kernel's device code unchanged?  Compiles csrc/*.hip files to gfx950 assembly twice - at a git
revision (the whole csrc/ and include/ of that revision, so header changes count) and in the working tree - with the flags
each tree's Makefile gives the file plus --cuda-device-only -S, and prints the diff.  Lines that contain __hip_cuid_ (a hash
of the translation unit) are ignored; any other difference exits non-zero.  No GPU needed.
    tools/isa_diff.py HEAD conv_x3.hip pack.hip [--defs=-DX3_EXP=7] [--jobs 4]"""
import argparse
import concurrent.futures
import difflib
import os
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join('gan_lab_amd', 'csrc')


def assembly(tree, name, defs, out):
    """Device assembly of `tree`/csrc/`name`, by the compile line of that tree's Makefile."""
    csrc = os.path.join(tree, CSRC)
    stem = name[:-len('.hip')]
    dry = subprocess.run(['make', '-n', '-B', '-C', csrc, f'DEFS={defs}', f'{stem}.o'], capture_output=True, text=True, check=True)
    line = next(ln for ln in dry.stdout.splitlines() if f' -c {name} ' in ln)
    cmd = shlex.split(line)
    i = cmd.index('-c')
    cmd[i:i + 4] = ['--cuda-device-only', '-S', name, '-o', out]      # replaces `-c file -o file.o`
    subprocess.run(cmd, cwd=csrc, check=True)
    with open(out) as f:
        return [ln for ln in f if '__hip_cuid_' not in ln]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('rev', help='git revision to compare the working tree against')
    ap.add_argument('files', nargs='+', help='file names under gan_lab_amd/csrc/')
    ap.add_argument('--defs', default='', help="the Makefile's DEFS (ablation builds)")
    ap.add_argument('--jobs', type=int, default=4)
    args = ap.parse_args()
    names = [os.path.basename(f) for f in args.files]
    changed = []
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, 'old')
        os.mkdir(old)
        tar = subprocess.run(['git', '-C', ROOT, 'archive', args.rev, CSRC, 'include'], capture_output=True, check=True).stdout
        subprocess.run(['tar', '-x', '-C', old], input=tar, check=True)
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            jobs = {n: (pool.submit(assembly, old, n, args.defs, os.path.join(tmp, n + '.old.s')),
                        pool.submit(assembly, ROOT, n, args.defs, os.path.join(tmp, n + '.new.s'))) for n in names}
            for n, (a, b) in jobs.items():
                a, b = a.result(), b.result()
                d = list(difflib.unified_diff(a, b, f'{args.rev}:{n}', n, n=2))
                sys.stdout.writelines(d)
                print(f'{n}: {len(b)} lines, ' + ('DIFFERENT' if d else 'identical'))
                if d:
                    changed.append(n)
    return 1 if changed else 0


if __name__ == '__main__':
    sys.exit(main())
