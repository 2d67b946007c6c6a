"""Static profile of the step workgroups' code in env_step_fused<Dyn, no EPA>, from their first barrier (in front of the per-env phase
P1) to the barrier behind the work pool: every instruction attributed to its source function through the line table (innermost inlined
location), so that what the HEAD of the P1 waves runs -- P1 and the set-up of the lanes' own first tickets: sincos, joint_of_step,
obstacle_of_step, fk_joint, the culling bounds, the end-effector read-out -- can be tabulated before and after a change, beside the
functions of the GJK trip, which such a change must leave as they are.  tools/loop_profile.py is the same method for one loop.
The compiler lays the blocks of this region out of source order, so the head is not a stretch of text: it is told apart by function.
Counts are static: a divergent branch counts once per side, a rolled loop once (the sincos loop of the set-up cache runs six times,
the chain of an own ticket `link` times).  The fused kernel holds the record-refill workgroups' code first and the step workgroups'
last; the step part has the kernel's last three barriers.  Diagnostic; usage:
    hipcc <flags of the Makefile> -gline-tables-only -S --cuda-device-only -o build/prof/dev.s urgym_hip.hip
    python tools/head_profile.py ur_gym_amd/csrc/build/prof/dev.s [mangled kernel symbol [directory of the sources it was built from]]"""
import bisect
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = sys.argv[2] if len(sys.argv) > 2 else '_ZN12_GLOBAL__N_114env_step_fusedILi2ELb0EEEvNS_7KParamsES1_PKfi'
lines = open(sys.argv[1]).read().split('\n')
start = [i for i, l in enumerate(lines) if l.startswith(SYMBOL + ':')][0]
end = [i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end')][0]
body = lines[start:end]
files = {}
for l in lines:
    m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m:
        files[int(m.group(1))] = (m.group(3) or m.group(2)).split('/')[-1]


def is_instruction(l):
    t = l.strip()
    return bool(t) and not (t.startswith('.') or t.startswith(';') or t.endswith(':'))


barriers = [i for i, l in enumerate(body) if l.strip().startswith('s_barrier')]
a, b = barriers[-3], barriers[-2]
SRC = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'ur_gym_amd/csrc')
hip = open(os.path.join(SRC, 'urgym_hip.hip')).read().split('\n')
dev = open(os.path.join(SRC, 'urgym_device.h')).read().split('\n')


def functions(src):
    return [(i, m.group(1)) for i, l in enumerate(src, 1) for m in [re.match(r'^\s*(?:template <[^>]*> )?__device__ (?:__forceinline__ )?.*?(\w+)\(', l)] if m]


fn = {'urgym_hip.hip': functions(hip), 'urgym_device.h': functions(dev)}


def fname(f, ln):
    if f in fn:
        k = bisect.bisect_right([x[0] for x in fn[f]], ln) - 1
        name = fn[f][k][1] if k >= 0 else '?'
        return ('hip:env_body:%d' % (ln // 20 * 20)) if name == 'env_body' else (('hip:' if f == 'urgym_hip.hip' else 'dev:') + name)
    return f  # (the math library's headers: sincos, sqrt, the divisions)


cur = None
per = collections.Counter()
kinds = collections.Counter()
for i, l in enumerate(body):
    m = re.match(r'\s*\.loc\s+(\d+)\s+(\d+)', l)
    if m:
        cur = (files.get(int(m.group(1)), '?'), int(m.group(2)))
        continue
    if i < a or i > b or not is_instruction(l):
        continue
    t = l.strip()
    per[fname(*cur) if cur else '?'] += 1
    kinds['vector' if t.startswith('v_') else ('scalar' if t.startswith('s_') else ('lds' if t.startswith('ds_') else 'memory'))] += 1
print('step workgroups, first barrier .. pool barrier: static instructions', sum(per.values()), dict(kinds))
print('whole kernel', sum(1 for l in body if is_instruction(l)))
for k, c in per.most_common(60):
    print('%-44s %5d' % (k, c))
