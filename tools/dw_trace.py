"""The single-part (precision 4) weight-gradient launches of the replayed P step, from a rocprofv3 kernel trace
(`*_kernel_trace.csv` of a short `bench.py` run, see tools/prof_streams.sh): every gemm_pp_kernel<..., K2> / gemm_pp_group_kernel
launch of ONE step with its grid (tiles x splits x products), start time relative to the step's head, duration and what else was
running while it ran, the split-K sums that finish them, and the family's total per step (median over the last steps).

    python3 tools/dw_trace.py /tmp/ps/s_kernel_trace.csv
"""
import collections
import csv
import sys


def short(n):
    return n.replace('(anonymous namespace)::', '').replace('void ', '')


def is_dw(n):          # gemm_pp_kernel<BM, 2, true, akm, bkm, true> (the K2 loop) and its grouped form
    if n.startswith('gemm_pp_group_kernel'):
        return True
    if not n.startswith('gemm_pp_kernel<'):
        return False
    a = [x.strip() for x in n[n.index('<') + 1:n.index('>')].split(',')]
    return len(a) >= 6 and a[1] == '2' and a[2] in ('true', '1') and a[5] in ('true', '1')


def is_sum(n):
    return n.startswith('splitk_sum_many_kernel') or n.startswith('splitk_reduce_kernel')


rows = []
for r in csv.DictReader(open(sys.argv[1])):
    wg = [max(int(r.get('Workgroup_Size_' + c, 1) or 1), 1) for c in 'XYZ']
    grid = tuple(int(r.get('Grid_Size_' + c, 0) or 0) // w for c, w in zip('XYZ', wg))
    rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), short(r['Kernel_Name']), grid, r.get('Queue_Id', '?')))
rows.sort()
heads = [i for i, r in enumerate(rows) if r[2].startswith('seed_word_kernel')]
steps = [rows[a:b] for a, b in zip(heads[:-1], heads[1:]) if b - a >= 500][-8:]
if not steps:
    print("no steps found (%d heads)" % len(heads))
    sys.exit(0)


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


tot = collections.defaultdict(list)
for ks in steps:
    t0, t1 = ks[0][0], max(k[1] for k in ks)
    tot['span'].append((t1 - t0) / 1e6)
    tot['dw'].append(sum(k[1] - k[0] for k in ks if is_dw(k[2])) / 1e6)
    tot['ndw'].append(sum(1 for k in ks if is_dw(k[2])))
    tot['sum'].append(sum(k[1] - k[0] for k in ks if is_sum(k[2])) / 1e6)
    tot['nsum'].append(sum(1 for k in ks if is_sum(k[2])))
    tot['dw_end'].append((max([k[1] for k in ks if is_dw(k[2]) or is_sum(k[2])] or [t0]) - t0) / 1e6)
print("steps analysed %d (medians): span %.3f ms; single-part GEMM launches %d, %.3f ms; split-K sums %d launches, %.3f ms; "
      "family + sums %.3f ms; last of them ends %.3f ms into the step" %
      (len(steps), med(tot['span']), med(tot['ndw']), med(tot['dw']), med(tot['nsum']), med(tot['sum']),
       med(tot['dw']) + med(tot['sum']), med(tot['dw_end'])))

ks = steps[-1]
t0 = ks[0][0]
print("\nlast step, launch by launch (grid = tiles x splits x products; 'with' = kernels overlapping it, by share of its duration):")
print("%9s %8s %-7s %-16s %-46s %s" % ("start us", "dur us", "queue", "grid", "kernel", "with"))
by_grid = collections.defaultdict(lambda: [0, 0.0])
for s, e, n, grid, q in ks:
    if not (is_dw(n) or is_sum(n)):
        continue
    over = collections.Counter()
    for s2, e2, n2, _, _ in ks:
        if (s2, e2, n2) != (s, e, n) and s2 < e and e2 > s:
            over[n2.split('<')[0].split('(')[0][:28]] += min(e, e2) - max(s, s2)
    w = ", ".join("%s %.0f%%" % (k, 100.0 * v / max(e - s, 1)) for k, v in over.most_common(3)) or "(alone)"
    print("%9.1f %8.1f %-7s %-16s %-46s %s" % ((s - t0) / 1e3, (e - s) / 1e3, q, "%dx%dx%d" % grid, n[:46], w))
    if is_dw(n):
        x = by_grid[(n[:46], grid)]
        x[0] += 1
        x[1] += (e - s) / 1e3
print("\nsingle-part launches of the last step by kernel and grid:")
for (n, grid), (c, t) in sorted(by_grid.items(), key=lambda kv: -kv[1][1]):
    print("  %-46s %-16s x%-3d %8.1f us  (avg %.1f)" % (n, "%dx%dx%d" % grid, c, t, t / c))
