"""Compare the two JSONs of tools/ab_wgrad_sweep.py (DIR/wgrad_parent.json, DIR/wgrad_new.json): the table rows under their own
state and the replayed problems.  Deterministic mode and everything in which ONE block owns each dW element must agree byte for
byte.  Where several blocks add to an element with fp32 atomics -- >= 2 splits, the four phases of a phase form, the row blocks of
the fp32 thin forms (the sweep's "split" list / "atomic" flag), or anything whose parent runs differ among themselves -- the result
is not reproducible even against itself: there the new library's first max |dw - dw64| has to lie within the parent's first three
figures, widened by their spread on each side (same kernel, same grid: only the order of the atomics can differ).  The parent's
own fourth run is held against the same range: how often a library misses the rule against itself.
usage: tools/ab_wgrad_compare.py DIR"""
import json
import sys

out = sys.argv[1]
a, b = json.load(open(f'{out}/wgrad_parent.json')), json.load(open(f'{out}/wgrad_new.json'))
ok = True
tally = {'atomic': 0, 'identical': 0, 'new outside': 0, 'parent outside': 0}


def ranged(name, sa, sb, p, q):
    """one atomic sum: shas and error figures of the parent (sa, p) and of the new library (sb, q)"""
    global ok
    tally['atomic'] += 1
    if len(set(sa + sb)) == 1:
        tally['identical'] += 1
        print(f'   {name}: byte-identical in all runs of both libraries')
        return
    if not p or not q or len(p) < 4:
        print(f'   {name}: NO ERROR FIGURES (parent {p}, new {q})')
        ok = False
        return
    spread = max(p[:3]) - min(p[:3])
    lo, hi = min(p[:3]) - spread, max(p[:3]) + spread
    inside, own = lo <= q[0] <= hi, lo <= p[3] <= hi
    tally['new outside'] += not inside
    tally['parent outside'] += not own
    print(f'   {name}: parent {" ".join(f"{v:.6e}" for v in p)} | new {" ".join(f"{v:.6e}" for v in q)} | [{lo:.6e}, {hi:.6e}] '
          f'new {"ok" if inside else "OUTSIDE"}, parent\'s 4th {"ok" if own else "OUTSIDE"}')
    ok &= inside


keys = list(a['deterministic'])
same = keys == list(b['deterministic'])
diff = [k for k in keys if a['deterministic'][k] != b['deterministic'].get(k)]
print(f'PROBLEMS deterministic: {len(keys)}, same problem list: {same}, differing: {len(diff)}')
for k in diff[:10]:
    print('   differs:', k)
ok &= same and not diff

keys = list(a['default'])
same = keys == list(b['default'])
split = set(b['split']) | {k for k in keys if len(set(a['default'][k])) != 1}
unsplit = [k for k in keys if k not in split]
diff = [k for k in unsplit if len(set(a['default'][k])) != 1 or a['default'][k] != b['default'].get(k)]
print(f'PROBLEMS default, one block per dW element: {len(unsplit)} (grouped items with one split included), same problem list: {same}, '
      f'differing: {len(diff)}')
for k in diff[:10]:
    print('   differs:', k, a['default'][k], b['default'].get(k))
ok &= same and not diff
print(f'PROBLEMS default, atomic sums: {len(split)}; max |dw - dw64|, parent x runs | new x runs | allowed range')
for k in [k for k in keys if k in split]:
    ranged(k, a['default'][k], b['default'][k], a['errors'].get(k), b['errors'].get(k))

ra, rb = a['rows'], b['rows']
same = list(ra) == list(rb)
owned = [k for k in ra if not rb[k]['atomic'] and len(set(ra[k]['sha'])) == 1]
diff = [k for k in owned if ra[k]['sha'] != rb[k]['sha']]
print(f'ROWS one block per dW element or deterministic workspace: {len(owned)} of {len(ra)}, same row list: {same}, differing: {len(diff)}')
for k in diff[:10]:
    print('   differs:', k)
ok &= same and not diff
print(f'ROWS atomic sums: {len(ra) - len(owned)}')
for k in [k for k in ra if k not in owned]:
    ranged('row ' + k, ra[k]['sha'], rb[k]['sha'], ra[k]['errors'], rb[k]['errors'])
print(f'ATOMIC SUMS: {tally}')
print('group:', a.get('group'), b.get('group'))
ok &= a.get('group') == b.get('group')
print('A/B', 'AGREES' if ok else 'DIFFERS')
sys.exit(0 if ok else 1)
