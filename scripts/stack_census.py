"""Census of the instruction stream of the encoder stack / chain kernels, by mnemonic class and loop level.

    python scripts/stack_census.py [--tree LABEL=CSRC_DIR ...] [--asm LABEL=FILE.s ...] [--out profiles/seam_census.md]

Compiles CSRC_DIR/encoder_chain.hip (default: one tree, `new=rohm_amd/csrc`) to gfx950 assembly with rohm_amd.build's flags -- nothing
runs on a GPU -- and counts, per kernel and per loop level, what a wave issues: MFMAs, accumulator moves, integer / address VALU, lane
moves, v_mov, s_nop, SALU, fp VALU, memory.  The trees are reported in the order given, so the parent commit goes first:

    git archive HEAD~1 rohm_amd/csrc include | tar -x -C /tmp/prev
    python scripts/stack_census.py --tree parent=/tmp/prev/rohm_amd/csrc --tree new=rohm_amd/csrc --out profiles/seam_census.md

Levels of encoder_stack_kernel<G>: the LAYER LOOP is the depth-1 loop with the most instructions; its "straight-line" code is every
block whose innermost loop is the layer loop itself (the seams: prologues, peeled chunks, epilogues, meetings, attention's
straight-line parts), "inner loops" is everything at depth >= 2, and "K loops" are the depth >= 2 blocks that hold MFMAs.  An MFMA-free
run is a maximal stretch of the layer loop's straight-line code, in layout order, without an MFMA.

It counts by mnemonic class only; it is not a search for particular instructions.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = ['mfma', 'accvgpr', 'int/address VALU', 'lane move', 'v_mov', 's_nop', 'SALU', 'fp VALU', 'other VALU', 'LDS', 'VMEM',
           'scalar load', 'wait/barrier/branch']
# the classes the seams should lose (ISSUE: none higher than the parent's, their sum lower)
OVERHEAD = ['int/address VALU', 'accvgpr', 'lane move', 'v_mov', 's_nop']

_INT = re.compile(r'v_(add|sub|subrev|addc|subb|subbrev)_(co_)?(ci_)?[ui](16|32|64)|v_(lshl|lshr|ashr|lshlrev|lshrrev|ashrrev)|v_(and|or|xor|not|xnor)(3)?_b|'
                  r'v_mul_(lo|hi|u32|i32)|v_mad_[ui]|v_bfe|v_bfi|v_bfm|v_bitop|v_and_or|v_or3|v_add3|v_xad|v_alignb|v_perm_b|v_cmp\w*_[ui](16|32|64)|'
                  r'v_(min|max|med3)3?_[ui]|v_mbcnt|v_sad|v_ffb|v_bcnt')
_FP = re.compile(r'v_\w+_f(16|32|64)|v_pk_|v_fma|v_exp|v_log|v_rcp|v_rsq|v_sqrt|v_sin|v_cos|v_cvt|v_ldexp|v_frexp|v_rndne|v_floor|v_ceil|v_trunc|v_fract')


def classify(m):
    if m.startswith('v_mfma') or m.startswith('v_smfma'):
        return 'mfma'
    if m.startswith('v_accvgpr'):
        return 'accvgpr'
    if m.startswith(('v_readlane', 'v_writelane')):
        return 'lane move'
    if m.startswith('v_mov'):
        return 'v_mov'
    if m == 's_nop':
        return 's_nop'
    if m.startswith(('s_waitcnt', 's_barrier', 's_branch', 's_cbranch', 's_endpgm', 's_sleep', 's_setprio', 's_sethalt', 's_trap')):
        return 'wait/barrier/branch'
    if m.startswith(('s_load', 's_buffer_load', 's_memrealtime', 's_memtime')):
        return 'scalar load'
    if m.startswith('s_'):
        return 'SALU'
    if m.startswith('ds_'):
        return 'LDS'
    if m.startswith(('global_', 'buffer_', 'scratch_', 'flat_')):
        return 'VMEM'
    if _INT.match(m):
        return 'int/address VALU'
    if _FP.match(m):
        return 'fp VALU'
    return 'other VALU'


class Block:
    def __init__(self):
        self.depth = 0
        self.header = None      # label of the innermost loop's header
        self.insts = []         # mnemonics, in order


_LABEL = re.compile(r'^(\.LBB\d+_\d+):')
_BB = re.compile(r'^; %bb\.\d+:')
_DEPTH = re.compile(r'Depth=(\d+)')
_INLOOP = re.compile(r'in Loop: Header=(BB\d+_\d+) Depth=(\d+)')
_INST = re.compile(r'^\t([a-z][a-z0-9_]*)\b')


def parse(asm_text):
    """-> {demangled-ish kernel name: [Block, ...]} for every kernel of the file"""
    kernels = collections.OrderedDict()
    cur = None
    blk = None
    in_header_comment = False
    for line in asm_text.splitlines():
        if line.startswith('_Z') and re.match(r'^_Z\w+:', line):
            name = line.split(':')[0]
            cur = kernels.setdefault(name, [])
            blk = Block()
            cur.append(blk)
            continue
        if cur is None:
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
            continue
        lab = _LABEL.match(line)
        if lab or _BB.match(line):
            blk = Block()
            cur.append(blk)
            in_header_comment = True
            if lab:
                blk.label = lab.group(1)[2:]
            tail = line
        elif in_header_comment and line.lstrip().startswith(';') and not line.startswith('\t;'):
            tail = line
        else:
            in_header_comment = False
            tail = None
        if tail is not None:
            m = _INLOOP.search(tail)
            if m:
                blk.header, blk.depth = m.group(1), int(m.group(2))
            elif 'Loop Header: Depth=' in tail:
                blk.depth = int(_DEPTH.search(tail).group(1))
                blk.header = getattr(blk, 'label', None)
            continue
        m = _INST.match(line)
        if m:
            blk.insts.append(m.group(1))
    return kernels


def short_name(mangled):
    m = re.match(r'_ZN4rohm(\d+)([a-z_0-9]+?)ILi(\d+)EEE', mangled)
    if m:
        return f'{m.group(2)[:int(m.group(1))]}<{m.group(3)}>'
    return mangled


def count(blocks):
    c = collections.Counter()
    for b in blocks:
        for m in b.insts:
            c[classify(m)] += 1
    return c


def census(blocks):
    """the levels of one kernel"""
    per_header = collections.Counter()
    for b in blocks:
        if b.depth == 1 and b.header:
            per_header[b.header] += len(b.insts)
    # the layer loop: the depth-1 loop whose straight-line code is the largest
    layer = per_header.most_common(1)[0][0] if per_header else None
    # blocks of deeper loops lie between the layer loop's blocks in layout order: everything from its first to its last block
    idx = [i for i, b in enumerate(blocks) if b.depth == 1 and b.header == layer]
    inside = blocks[idx[0]:idx[-1] + 1] if idx else []
    straight = [b for b in inside if b.depth == 1]
    inner = [b for b in inside if b.depth >= 2]
    kloops = [b for b in inner if any(m.startswith('v_mfma') for m in b.insts)]
    outside = [b for b in blocks if b not in inside]
    runs = []
    run = 0
    for b in inside:
        if b.depth >= 2:
            if b in kloops and run:
                runs.append(run)
                run = 0
            continue
        for m in b.insts:
            if m.startswith('v_mfma'):
                if run:
                    runs.append(run)
                run = 0
            else:
                run += 1
    if run:
        runs.append(run)
    return {'layer straight-line': count(straight), 'layer inner loops': count(inner), 'K loops': count(kloops), 'outside the layer loop': count(outside),
            'whole kernel': count(blocks), 'runs': sorted((r for r in runs if r >= 120), reverse=True), 'runs_all': sum(r for r in runs if r >= 120)}


def compile_asm(csrc):
    from rohm_amd import build
    hipcc = build.find_hipcc()
    if hipcc is None:
        raise SystemExit('hipcc not found')
    flags = [f'--offload-arch={build.ARCH}', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result']
    with tempfile.TemporaryDirectory(prefix='rohm_census_') as tmp:
        out = os.path.join(tmp, 'encoder_chain.s')
        r = subprocess.run([hipcc] + flags + ['--cuda-device-only', '-S', 'encoder_chain.hip', '-o', out, '-Rpass-analysis=kernel-resource-usage'],
                           cwd=csrc, stderr=subprocess.PIPE, text=True, check=True)
        return open(out).read(), r.stderr


def resources(remarks):
    """{kernel: 'VGPRs 256, AGPRs 256, ...'} from -Rpass-analysis=kernel-resource-usage"""
    res, name = collections.OrderedDict(), None
    for line in remarks.splitlines():
        m = re.search(r'remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\S+)', line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            name = short_name(m.group(2))
            res[name] = []
        elif name:
            res[name].append(f'{m.group(1)} {m.group(2)}')
    return {k: ', '.join(v) for k, v in res.items()}


def report(label, asm_text, remarks):
    out = [f'## {label}', '']
    res = resources(remarks) if remarks else {}
    for mangled, blocks in parse(asm_text).items():
        name = short_name(mangled)
        c = census(blocks)
        out += [f'### `{name}` ({label})', '']
        if name in res:
            out += [f'Resources: {res[name]}.', '']
        levels = ['layer straight-line', 'layer inner loops', 'K loops', 'outside the layer loop', 'whole kernel']
        out += ['| class | ' + ' | '.join(levels) + ' |', '|---|' + '---|' * len(levels)]
        for cl in CLASSES:
            out.append(f'| {cl} | ' + ' | '.join(str(c[lv][cl]) for lv in levels) + ' |')
        out.append('| **all** | ' + ' | '.join(str(sum(c[lv].values())) for lv in levels) + ' |')
        out.append('| **seam overhead** (' + ' + '.join(OVERHEAD) + ') | ' + ' | '.join(str(sum(c[lv][k] for k in OVERHEAD)) for lv in levels) + ' |')
        out += ['', f'MFMA-free runs of >= 120 instructions in the layer loop: {len(c["runs"])}, {c["runs_all"]} instructions in all: ' +
                ', '.join(str(r) for r in c['runs']) + '.', '']
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--tree', action='append', default=[], metavar='LABEL=CSRC_DIR')
    ap.add_argument('--asm', action='append', default=[], metavar='LABEL=FILE.s', help='count an assembly file that exists already')
    ap.add_argument('--out', default=None, help='write the report here (default: print it)')
    ap.add_argument('--preamble', default=None, help='a markdown file put in front of the tables')
    a = ap.parse_args()
    if not a.tree and not a.asm:
        a.tree = ['new=' + os.path.join(ROOT, 'rohm_amd', 'csrc')]
    parts = ['# Instruction census of the encoder stack and chain kernels (scripts/stack_census.py)', '',
             'Instructions per kernel by class and loop level, from the gfx950 assembly of `encoder_chain.hip` built with the shipped flags.'
             ' The layer loop executes once per layer: its straight-line column is what a wave issues per layer between and around the K loops.', '']
    if a.preamble:
        parts += [open(a.preamble).read().rstrip(), '']
    for spec in a.tree:
        label, path = spec.split('=', 1)
        text, remarks = compile_asm(os.path.abspath(path))
        parts.append(report(label, text, remarks))
    for spec in a.asm:
        label, path = spec.split('=', 1)
        parts.append(report(label, open(path).read(), None))
    text = '\n'.join(parts) + '\n'
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == '__main__':
    main()
