#!/usr/bin/env python3
"""Instruction mix of one kernel in a hipcc -save-temps .s file: python scripts/asm_mix.py file.s kernel-name-substring
With --lds-waits: for EVERY kernel whose name holds the substring, one line with
  - the returning LDS atomics (ds_*_rtn_*) and how many of them have a full `s_waitcnt lgkmcnt(0)` as the very next instruction;
  - the LDS-DMA requests (global_load_lds_*), and the `s_waitcnt` with a vmcnt field that stand directly in front of a ds_*
    instruction (how the compiler orders LDS accesses behind an LDS-DMA it knows of; block placement makes "between the requests
    and the barrier" unreadable from the text order, so the waits are counted where they are put)."""
import re
import sys
from collections import Counter


def kernels(src, key):
    """(label line, instruction lines) of every kernel whose label holds `key`"""
    for i, l in enumerate(src):
        if key in l and l.rstrip().split(';')[0].rstrip().endswith(':') and not l.startswith(('\t', ' ')):
            end = next(j for j in range(i, len(src)) if 's_endpgm' in src[j])
            ins = []
            for m in src[i + 1:end]:
                t = m.strip().split()
                if not t or t[0].startswith(('.', ';')) or t[0].endswith(':'):
                    continue
                ins.append(m.strip())
            yield l, ins


def lds_waits(label, ins):
    op = [m.split()[0] for m in ins]
    rtn = [i for i, o in enumerate(op) if re.match(r'ds_\w+_rtn_', o)]
    at_once = sum(1 for i in rtn if i + 1 < len(ins) and op[i + 1] == 's_waitcnt' and 'lgkmcnt(0)' in ins[i + 1])
    dma = sum(1 for o in op if o.startswith('global_load_lds_'))
    # the waitcnt pass orders a ds_* behind an LDS-DMA it knows of by a vmcnt wait directly in front of it
    vm_ds = sum(1 for i, o in enumerate(op[:-1]) if o == 's_waitcnt' and 'vmcnt' in ins[i] and op[i + 1].startswith('ds_'))
    vm_atom = sum(1 for i, o in enumerate(op[:-1]) if o == 's_waitcnt' and 'vmcnt' in ins[i] and re.match(r'ds_(or|add)_', op[i + 1]))
    print('%-62s rtn LDS atomics %3d, waited for at once %3d | LDS-DMA requests %d, vmcnt waits in front of a ds_* %3d (of an LDS atomic: %3d)' % (
        label.split(':')[0][:62], len(rtn), at_once, dma, vm_ds, vm_atom))


def mix(label, ins):
    c = Counter()
    for l in ins:
        op = l.split()[0]
        c[op.split('_')[0]] += 1
        if 'dpp' in l:
            c['(dpp)'] += 1
        if op.startswith('v_') and ('b64' in op or 'u64' in op or 'mul_lo' in op or 'mad_u64' in op or 'f64' in op):
            c['(half-rate valu)'] += 1
    print(label[:80])
    print(len(ins), 'instructions', dict(c))


if __name__ == '__main__':
    src = open(sys.argv[1]).read().split('\n')
    found = list(kernels(src, sys.argv[2]))
    if '--lds-waits' in sys.argv[3:]:
        for label, ins in found:
            lds_waits(label, ins)
    else:
        mix(*found[0])
