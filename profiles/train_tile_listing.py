"""What the compiler made of the train step's four persistent-kernel files in two source trees, instantiation by instantiation
(29: 16 forward recurrences, 4 backward recurrences, 3 attention cells, 3 + 3 attention-cell backward and its rows kernel).

    python profiles/train_tile_listing.py [--parent REV_OR_DIR] [--out profiles/train_tile_listing.txt]

The parent tree is a directory that holds cor_asv_ann_amd/csrc and include, or a git revision exported to a temporary one
(default HEAD^).  Both trees are compiled device-only for gfx950 with csrc/Makefile's flags, as csrc/check_asm_loads.py obtains
its listing.  Per kernel one line: `identical` when the instruction text is the same (comment lines, .file and .ident apart);
otherwise the figures of both trees (VGPRs, AGPRs, SGPRs, LDS, scratch, spills) and the diff of the ordered sequence of matrix,
LDS, global-memory, barrier and wait instructions.  figures() and sequence() are also what tests/test_train_tile_static.py holds
this tree to.  The c4 timing covers W = 512 alone; for the W = 128 and W = 256 instantiations this report is the check."""
import argparse
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ['train_persist.hip', 'train_persist_bwd.hip', 'train_persist_top.hip', 'train_persist_topb.hip']
HIPCC = os.environ.get('HIPCC') or '/opt/rocm/bin/hipcc'
FIGURES = ['vgpr_count', 'agpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size', 'vgpr_spill_count',
           'sgpr_spill_count']
ORDERED = re.compile(r'^(v_mfma\w*|ds_\w+|global_\w+|buffer_\w+|scratch_\w+|flat_\w+|s_barrier|s_waitcnt)\b')


def listing(tree, name, tmp):
    """The gfx950 ISA listing of csrc/<name> in `tree`."""
    csrc = os.path.join(tree, 'cor_asv_ann_amd', 'csrc')
    out = os.path.join(tmp, '%s.%s.s' % (hashlib.sha1(tree.encode()).hexdigest()[:8], name))
    subprocess.run([HIPCC, '-O3', '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-S', '-I' + os.path.join(tree, 'include'),
                    os.path.join(csrc, name), '-o', out], check=True, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    with open(out) as f:
        return f.read()


def short(mangled):
    m = re.search(r'casv\d+(\w+_kernel)ILi(\d+)E', mangled)
    return '%s<%s>' % (m.group(1), m.group(2)) if m else mangled


def kernels(text):
    """{kernel<NT>: instruction text, a list of lines} of a listing: comment lines, .file and .ident left out."""
    out, name = {}, None
    for raw in text.split('\n'):
        t = raw.strip()
        m = re.match(r'^(_Z\w+):', t)
        if m:
            name = short(m.group(1))
            out[name] = []
        elif name is not None:
            if t.startswith('.Lfunc_end'):
                name = None
            elif t and not t.startswith((';', '.file', '.ident')):
                out[name].append(t)
    return out


def figures(text):
    """{kernel<NT>: {figure: value}} from the listing's kernel metadata."""
    meta = text[text.index('amdhsa.kernels'):]
    out = {}
    for block in re.split(r'\n  - \.agpr_count', meta)[1:]:
        block = '.agpr_count' + block
        name = short(re.search(r'\.name:\s+(\S+)', block).group(1))
        out[name] = {k: int(re.search(r'\.%s:\s+(\d+)' % k, block).group(1)) for k in FIGURES}
    return out


def sequence(lines, waits=True):
    """The ordered matrix, LDS, memory, barrier (and wait) instructions of a kernel: mnemonic and modifiers, registers left out."""
    out = []
    for t in lines:
        m = ORDERED.match(t)
        if not m or (m.group(1) == 's_waitcnt' and not waits):
            continue
        mods = re.findall(r'offset:\d+|\bsc[01]\b|\bnt\b|vmcnt\(\d+\)|lgkmcnt\(\d+\)|expcnt\(\d+\)|cbsz:\d+|abid:\d+|blgp:\d+|\boff\b', t)
        out.append(' '.join([m.group(1)] + mods))
    return out


def sequence_digest(lines):
    return hashlib.sha256('\n'.join(sequence(lines, waits=False)).encode()).hexdigest()[:16]


def wait_differences(a, b):
    """The s_waitcnt differences of two kernels whose other ordered instructions agree: (what, where) with `where` the ordinal
    and text of the ordered instructions around it, and `in chain` when matrix instructions stand on both sides."""
    sa, sb = sequence(a), sequence(b)
    out = []
    sm = difflib.SequenceMatcher(None, sa, sb, autojunk=False)
    for tag, i0, i1, j0, j1 in sm.get_opcodes():
        if tag == 'equal':
            continue
        before = next((x for x in reversed(sb[:j0]) if not x.startswith('s_waitcnt')), 'entry')
        after = next((x for x in sb[j1:] if not x.startswith('s_waitcnt')), 'end')
        chain = any(x.startswith('v_mfma') for x in sb[:j0]) and any(x.startswith('v_mfma') for x in sb[j1:])
        out.append('parent %s -> here %s, at #%d after `%s` before `%s`%s'
                   % (sa[i0:i1] or 'nothing', sb[j0:j1] or 'nothing', j0, before, after, ' (matrix instructions on both sides)' if chain else ''))
    return out


def report(parent, here, files=FILES):
    lines, bad = [], 0
    lines.append('# parent tree against this one, per kernel instantiation.  Required: LDS, scratch and spill counts equal, vgpr_count + agpr_count')
    lines.append('# not above the parent\'s, the ordered sequence of matrix, LDS, memory and barrier instructions identical; every s_waitcnt')
    lines.append('# difference is listed with the ordinal and the neighbours it has in the ordered sequence.  A kernel\'s text is its time loop, so')
    lines.append('# "matrix instructions on both sides" holds for whatever sits in the loop: a stage chain runs from the first ds_write_b128 after')
    lines.append('# the run of sc1 loads to the barrier behind the last v_mfma, and no difference below adds a wait there.  c4 times W = 512 alone:')
    lines.append('# for the NT = 4 and NT = 8 instantiations this report is the check.')
    with tempfile.TemporaryDirectory() as tmp:
        for name in files:
            tp, th = listing(parent, name, tmp), listing(here, name, tmp)
            kp, kh, fp, fh = kernels(tp), kernels(th), figures(tp), figures(th)
            assert sorted(kp) == sorted(kh), (name, sorted(kp), sorted(kh))
            for k in sorted(kp, key=lambda s: (s.split('<')[0], int(s.split('<')[1][:-1]))):
                if kp[k] == kh[k] and fp[k] == fh[k]:
                    lines.append('%-22s %-42s identical (%d instructions)' % (name, k, len(kp[k])))
                    continue
                same_seq = sequence(kp[k], False) == sequence(kh[k], False)
                ok = (same_seq and all(fp[k][f] == fh[k][f] for f in FIGURES[3:])
                      and fh[k]['vgpr_count'] + fh[k]['agpr_count'] <= fp[k]['vgpr_count'] + fp[k]['agpr_count'])
                bad += not ok
                lines.append('%-22s %-42s %s' % (name, k, 'differs: figures and ordered sequence hold' if ok else 'DIFFERS: requirement missed'))
                lines.append('    parent ' + ' '.join('%s=%d' % (f, fp[k][f]) for f in FIGURES))
                lines.append('    here   ' + ' '.join('%s=%d' % (f, fh[k][f]) for f in FIGURES))
                if same_seq:
                    waits = wait_differences(kp[k], kh[k])
                    lines += ['    wait: ' + w for w in waits] or ['    ordered sequence identical, waits included (scalar / address arithmetic differs)']
                else:
                    lines += ['    ' + d for d in difflib.unified_diff(sequence(kp[k]), sequence(kh[k]), 'parent', 'here', lineterm='', n=2)]
    lines.append('%d instantiations, %d miss a requirement' % (sum(1 for ln in lines if ln[:1] not in ' #'), bad))
    return lines, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('files', nargs='*', default=FILES, help='a subset of the four files')
    ap.add_argument('--parent', default='HEAD^')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_tile_listing.txt'))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        parent = a.parent
        if not os.path.isdir(parent):
            tar = subprocess.run(['git', '-C', ROOT, 'archive', a.parent, 'cor_asv_ann_amd/csrc', 'include'], check=True, stdout=subprocess.PIPE)
            subprocess.run(['tar', '-x', '-C', tmp], input=tar.stdout, check=True)
            parent = tmp
        lines, bad = report(os.path.abspath(parent), ROOT, a.files)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
