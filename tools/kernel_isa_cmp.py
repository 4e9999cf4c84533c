"""Compare two builds of the same HIP sources kernel by kernel: did a source-level refactor change the code objects?

Each build directory holds, per object, a sub-directory with `remarks.txt` (the stderr of a hipcc line that carried
-Rpass-analysis=kernel-resource-usage) and the `*-gfx950.s` that --save-temps leaves.  For every kernel the resource figures
(VGPRs, AGPRs, SGPRs, scratch, LDS, occupancy) are compared, then the instruction streams after stripping comments, directives,
debug lines and label / function numbering.  Kernels whose instructions differ are listed with instruction counts by class
(MFMA, VALU, ds_*, global_*, s_waitcnt, and the s_waitcnt vmcnt(0) among them).

Usage: kernel_isa_cmp.py PARENT_DIR TREE_DIR > table.txt     (exit status 1 if any resource figure differs)"""
import collections
import glob
import os
import re
import sys

FIELDS = ('VGPRs', 'AGPRs', 'TotalSGPRs', 'ScratchSize [bytes/lane]', 'LDS Size [bytes/block]', 'Occupancy [waves/SIMD]')


def resources(path):
    out, cur = {}, None
    for line in open(path, errors='replace'):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r':\s+([A-Za-z][^:]*): (\S+) \[-Rpass-analysis', line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            cur[m.group(1).strip()] = m.group(2)
    return out


def streams(path):
    """kernel / function name -> its normalised instruction list"""
    out, name = {}, None
    for line in open(path, errors='replace'):
        if name is None:
            m = re.match(r'^(_Z\w+):', line)
            if m:
                name, out[m.group(1)] = m.group(1), []
            continue
        if line.startswith('.Lfunc_end'):
            name = None
            continue
        s = line.split(';')[0].strip()
        if not s or s.startswith('.'):
            continue
        out[name].append(re.sub(r'\.L[A-Za-z_]*\d+_(\d+)', r'.L_\1', ' '.join(s.split())))
    return out


def classes(insts):
    c = collections.Counter()
    for s in insts:
        op = s.split()[0]
        if op.startswith('v_mfma'):
            c['mfma'] += 1
        elif op.startswith('v_'):
            c['valu'] += 1
        elif op.startswith('ds_'):
            c['ds'] += 1
        elif op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
            c['global'] += 1
        elif op.startswith('s_waitcnt'):
            c['waitcnt'] += 1
            if re.search(r'vmcnt\(0\)', s):
                c['vmcnt0'] += 1
    return ' '.join('%s %d' % (k, c[k]) for k in ('mfma', 'valu', 'ds', 'global', 'waitcnt', 'vmcnt0'))


def main():
    parent, tree = sys.argv[1], sys.argv[2]
    bad_res, n_kernels, n_same, differ = 0, 0, 0, []
    print('%-16s %-100s %s' % ('object', 'kernel', ' | '.join(FIELDS)))
    for obj in sorted(os.listdir(parent)):
        pr, tr = os.path.join(parent, obj, 'remarks.txt'), os.path.join(tree, obj, 'remarks.txt')
        if not (os.path.isfile(pr) and os.path.isfile(tr)):
            continue
        rp, rt = resources(pr), resources(tr)
        sp = streams(glob.glob(os.path.join(parent, obj, '*gfx950.s'))[0])
        st = streams(glob.glob(os.path.join(tree, obj, '*gfx950.s'))[0])
        for k in sorted(set(rp) | set(rt)):
            n_kernels += 1
            a, b = rp.get(k), rt.get(k)
            if a is None or b is None:
                bad_res += 1
                print('%-16s %-100s ONLY IN %s' % (obj, k, 'PARENT' if b is None else 'TREE'))
                continue
            same = a == b
            bad_res += not same
            print('%-16s %-100s %s%s' % (obj, k, ' | '.join(b.get(f, '?') for f in FIELDS),
                                        '' if same else '   PARENT: ' + ' | '.join(a.get(f, '?') for f in FIELDS)))
            if sp.get(k) == st.get(k):
                n_same += 1
            else:
                differ.append((obj, k, classes(sp.get(k, [])), classes(st.get(k, []))))
    print()
    print('%d kernels; resource figures differ in %d; instruction streams identical in %d, different in %d' %
          (n_kernels, bad_res, n_same, len(differ)))
    for obj, k, a, b in differ:
        print('  %s %s\n    parent: %s\n    tree:   %s' % (obj, k, a, b))
    return 1 if bad_res else 0


if __name__ == '__main__':
    sys.exit(main())
