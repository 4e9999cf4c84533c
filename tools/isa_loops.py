"""Loops of one kernel of a hipcc -S listing: every backward branch closes a loop [target label .. branch]; per loop the MFMA count of
each basic block in it, the vector stores to global memory, the full drains (s_waitcnt vmcnt(0)) and the conditional branches.  What a K
loop should show: the MFMA block sizes of its rider-less sibling, no store, no full drain.  (tools/isa_mix.py gives the instruction
mix of the same blocks.)  Usage: isa_loops.py listing.s <mangled-name-substring> [min_mfma_per_loop]"""
import re
import sys

path, key = sys.argv[1], sys.argv[2]
min_mfma = int(sys.argv[3]) if len(sys.argv) > 3 else 1
lines = open(path).read().split('\n')
start = next(i for i, l in enumerate(lines) if l.startswith('_Z') and key in l and l.rstrip().split(':')[0].endswith('E') and ':' in l)
end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))

blocks, pos = [], {}          # [name, mfma, stores, drains, cbranch, branch targets]
cur = ['entry', 0, 0, 0, 0, []]
for l in lines[start + 1:end]:
    s = l.strip()
    if not s or s.startswith(';'):
        continue
    m = re.match(r'^(\.LBB\w+):', s)
    if m:
        blocks.append(cur)
        cur = [m.group(1), 0, 0, 0, 0, []]
        continue
    if s.startswith('.'):
        continue
    op = s.split()[0]
    if op.startswith('v_mfma'):
        cur[1] += 1
    elif op.startswith(('global_store', 'buffer_store', 'flat_store', 'global_atomic')):
        cur[2] += 1
    elif op.startswith('s_waitcnt') and re.search(r'vmcnt\(0\)', s):
        cur[3] += 1
    elif op.startswith(('s_cbranch', 's_branch')):
        cur[4] += op.startswith('s_cbranch')
        cur[5].append(s.split()[1])
blocks.append(cur)
for i, b in enumerate(blocks):
    pos[b[0]] = i

loops = set()
for i, b in enumerate(blocks):
    for t in b[5]:
        if t in pos and pos[t] <= i:
            loops.add((pos[t], i))
print('%-14s %-14s %6s %6s %6s %6s  MFMAs per block' % ('loop head', 'back edge', 'mfma', 'store', 'drain', 'cbr'))
for h, t in sorted(loops):
    body = blocks[h:t + 1]
    mf = sum(b[1] for b in body)
    if mf < min_mfma:
        continue
    print('%-14s %-14s %6d %6d %6d %6d  %s' % (blocks[h][0], blocks[t][0], mf, sum(b[2] for b in body), sum(b[3] for b in body),
                                                 sum(b[4] for b in body), ' / '.join(str(b[1]) for b in body if b[1])))
for l in lines[end:end + 60]:
    if any(k in l for k in ('NumVgprs', 'ScratchSize', 'Occupancy')):
        print(l.strip())
