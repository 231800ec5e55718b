#!/usr/bin/env python3
"""Static check of the store epilogue of the bf16-split GEMM kernels (csrc/gemm.hip: k_gemm_bx3, k_gemm_bx3w, k_gemm_bx3h --
every instantiation) on a fresh `hipcc -S`.

A wave stores its 64 x 64 sub-tile in passes: one `ds_read_b128` of a transposed row segment, the epilogue's arithmetic, the
row store.  On gfx950 `vmcnt` counts stores as well as loads, so a vector-memory load inside a pass -- or any `s_waitcnt` that
names vmcnt -- makes the pass wait for the previous pass's stores: the store tail runs one pass at a time.  What must hold on the
final ISA, behind the kernel's last MFMA:

  from the LDS read that opens the first store pass to the last store of the last pass there is no `global_load` / `buffer_load` and no
  `s_waitcnt` naming vmcnt -- not between a pass's LDS read and its row store, and not from there to the next pass's LDS read.

One exception, for the forward-only cross entropy (EM = 1) only: its eight target ids per block of eight passes are loaded
and waited for ONCE per block, in the gap between the last store of a block and the first LDS read of the next one, i.e. where
the transpose's `ds_write`s are.  A load or vmcnt wait there is counted as `blk` and allowed; anywhere else it is a problem.

Per instantiation the tool prints: vector-memory loads and vmcnt waits between the last MFMA and the end of the last store pass, how
many of those lie in front of the first pass (`front`: the bias load and its one wait, what the k loop left behind it), inside the
pass region (`in`, must be 0) or in a block gap (`blk`),
the store passes found, VGPRs, AGPRs, scratch bytes and the occupancy the compiler reports.  Scratch must be 0, and k_gemm_bx3h
must keep 2 waves per SIMD.

  check_gemm_epilogue_asm.py            compile csrc/gemm.hip and check it
  check_gemm_epilogue_asm.py --asm F    check an ISA listing made earlier (e.g. of another commit)

Exit code 0 = ok.  Used by tests/test_gemm_epilogue_asm.py (CPU box: hipcc cross-compiles without a GPU).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'few-shot-music-generation_amd', 'csrc')
# template arguments per kernel when the epilogue's mode is one of them (the last)
NARGS = {'k_gemm_bx3': 5, 'k_gemm_bx3w': 6, 'k_gemm_bx3h': 7}
MODES = {0: 'plain', 1: 'ce_fwd', 2: 'ce_store'}
OPER = {0: 'KC', 1: 'XC'}


def kernels(asm):
    """[(kernel, template args, body lines, footer comment text)] of every bf16-split GEMM instantiation, in file order"""
    out = []
    for m in re.finditer(r'^(_ZN4fsmg\S*?\d+(k_gemm_bx3[wh]?)I(\S*?)EEvNS_8GemmArgsE):\s', asm, re.M):
        end = asm.index('.end_amdhsa_kernel', m.end())
        stop = asm.index('.Lfunc_end', m.end())
        foot = asm[end:end + 4000]
        args = [int(a) for a in re.findall(r'L[ib](\d+)E', m.group(3) + 'E')]
        out.append((m.group(2), args, asm[m.end():stop].splitlines(), foot))
    return out


def describe(kern, args):
    has_mode = len(args) == NARGS[kern]
    mode = args[-1] if has_mode else None
    a = list(args[:-1] if has_mode else args)
    names = {'k_gemm_bx3': ['PROF', 'BUFM'], 'k_gemm_bx3w': ['MT', 'PROF', 'BUFM'], 'k_gemm_bx3h': ['PROF', 'BUFM', 'QUEUE', 'AG']}[kern]
    text = '%s<%s,%s' % (kern, OPER[a[0]], OPER[a[1]])
    for n, v in zip(names, a[2:]):
        if n == 'BUFM' or n == 'MT':
            text += ' %s=%d' % (n, v)
        elif v:
            text += ' ' + n
    text += ' | ' + (MODES[mode] if has_mode else 'run-time mode') + '>'
    return text, mode


def check(kern, mode, lines, foot):
    code = []
    for raw in lines:
        line = raw.split(';')[0].strip()
        if line and not line.startswith('.') and not line.endswith(':'):
            code.append(line)
    mfma = [i for i, l in enumerate(code) if l.startswith('v_mfma')]
    if not mfma:
        return None, ['no MFMA found']
    tail = code[mfma[-1] + 1:]
    is_load = lambda l: l.startswith(('global_load', 'buffer_load', 'flat_load', 'scratch_load'))
    is_wait = lambda l: l.startswith('s_waitcnt') and 'vmcnt' in l
    reads = [i for i, l in enumerate(tail) if l.startswith('ds_read_b128')]
    problems = []
    # 2 blocks of 8 passes per 64 x 64 sub-tile; a wave of k_gemm_bx3h stores two of them.  Exactly: a change of code layout that puts
    # other b128 reads (slow paths of the k loop) behind the last MFMA must fail here, not shift the window
    want = 32 if kern == 'k_gemm_bx3h' else 16
    if len(reads) != want:
        problems.append('%d store passes found behind the last MFMA, expected %d' % (len(reads), want))
    inside = blk = 0
    is_store = lambda l: l.startswith(('global_store', 'buffer_store'))
    if len(reads) >= 2:
        # the passes are unrolled copies: the last one ends behind as many stores as the one in front of it holds (what follows in
        # the file is other code of the kernel -- loader waves, slow paths of the k loop --, not the epilogue)
        per_pass = sum(1 for l in tail[reads[-2]:reads[-1]] if is_store(l))
        end, seen = reads[-1], 0
        while end < len(tail) and seen < per_pass:
            seen += is_store(tail[end])
            end += 1
        if seen < per_pass or per_pass == 0:
            problems.append('the end of the last store pass was not found')
        tail = tail[:end]
        for k in range(reads[0], len(tail)):
            l = tail[k]
            if not (is_load(l) or is_wait(l)):
                continue
            prev = max(r for r in reads if r <= k)
            nxt = min([r for r in reads if r > k] or [len(tail)])
            gap = any(x.startswith('ds_write') for x in tail[prev:nxt])
            stores_follow = any(is_store(x) for x in tail[k:nxt])
            if mode == 1 and gap and nxt < len(tail) and not stores_follow:
                blk += 1
            else:
                inside += 1
                if inside <= 4:
                    problems.append('pass %d: "%s" inside the store passes' % (reads.index(prev), l))
        if inside > 4:
            problems.append('... %d loads / vmcnt waits inside the store passes in all' % inside)

    first = reads[0] if reads else 0
    n_load = sum(1 for l in tail if is_load(l))          # behind the last MFMA, to the end of the last pass
    n_wait = sum(1 for l in tail if is_wait(l))
    n_front = sum(1 for l in tail[:first] if is_load(l) or is_wait(l))

    def num(key):
        m = re.search(r';\s*%s:\s*(\d+)' % key, foot)
        return int(m.group(1)) if m else -1
    vgpr, agpr, scratch, occ = num('NumVgprs'), num('NumAgprs'), num('ScratchSize'), num('Occupancy')
    if scratch != 0:
        problems.append('scratch is %d bytes, must be 0' % scratch)
    if kern == 'k_gemm_bx3h' and occ < 2:
        problems.append('occupancy %d waves per SIMD, k_gemm_bx3h needs 2' % occ)
    row = (n_load, n_wait, n_front, inside, blk, len(reads), vgpr, agpr, scratch, occ)
    return row, problems


def main(argv):
    if len(argv) >= 2 and argv[0] == '--asm':
        asm = open(argv[1]).read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, 'gemm.s')
            hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
            cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '--cuda-device-only', '-S',
                   os.path.join(CSRC, 'gemm.hip'), '-o', out]
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
            if proc.returncode != 0:
                print(proc.stdout)
                return 2
            asm = open(out).read()
    ks = kernels(asm)
    if len(ks) < 34:
        print('expected at least 34 bf16-split GEMM instantiations, found %d' % len(ks))
        return 1
    print('%-58s %5s %5s %5s %4s %4s %6s %5s %5s %7s %4s' % ('instantiation', 'loads', 'waits', 'front', 'in', 'blk', 'passes', 'vgpr', 'agpr', 'scratch', 'occ'))
    bad = 0
    notes = []
    for kern, args, lines, foot in ks:
        text, mode = describe(kern, args)
        row, problems = check(kern, mode, lines, foot)
        if row is not None:
            print('%-58s %5d %5d %5d %4d %4d %6d %5d %5d %7d %4d' % ((text,) + row))
        else:
            print('%-58s %s' % (text, problems[0]))
        for p in problems:
            notes.append('%s: %s' % (text, p))
        bad += len(problems)
    for n in notes:
        print('   ' + n)
    print('%d instantiations, %s' % (len(ks), 'ok' if not bad else '%d problem(s)' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
