"""Compare the two sweep JSONs of tools/ab_conv_sweep.py (output bytes: DIR/sweep_parent.json, DIR/sweep_new.json) and the two
rocprofv3 --kernel-trace CSVs of the same sweep (DIR/kt_parent, DIR/kt_new: kernel names, grids, workgroups, LDS in launch order).
usage: tools/ab_conv_compare.py DIR"""
import csv
import glob
import json
import sys

out = sys.argv[1]
a, b = json.load(open(f'{out}/sweep_parent.json')), json.load(open(f'{out}/sweep_new.json'))
ok = True
for mode in ('default', 'deterministic'):
    keys = list(a[mode])
    same_keys = keys == list(b[mode])
    diff = [k for k in keys if a[mode][k] != b[mode].get(k)]
    ns = sum(1 for k in keys if a[mode][k] == 'not served')
    print(f'BYTES {mode}: {len(keys)} problems, same problem list: {same_keys}, differing outputs: {len(diff)}, not served (both): {ns}')
    for k in diff[:10]:
        print('   differs:', k)
    ok &= same_keys and not diff


def trace(tag):
    files = glob.glob(f'{out}/kt_{tag}/**/*kernel_trace.csv', recursive=True)
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    cols = [c for c in rows[0] if c in ('Kernel_Name', 'Grid_Size_X', 'Grid_Size_Y', 'Grid_Size_Z', 'Workgroup_Size_X', 'LDS_Block_Size',
                                        'Grid_Size', 'Workgroup_Size', 'LDS_Block_Size_v', 'Scratch_Size', 'Private_Segment_Size')]
    return [tuple(r[c] for c in cols) for r in rows], cols


ta, cols = trace('parent')
tb, _ = trace('new')
conv_a = [r for r in ta if 'conv' in r[0]]
conv_b = [r for r in tb if 'conv' in r[0]]
print(f'DISPATCH columns compared: {cols}')
print(f'DISPATCH all kernels: parent {len(ta)}, new {len(tb)}, identical sequence: {ta == tb}')
print(f'DISPATCH conv kernels: parent {len(conv_a)}, new {len(conv_b)}, identical sequence: {conv_a == conv_b}, '
      f'distinct (name, grid, lds): {len(set(conv_a))}')
if conv_a != conv_b:
    for i, (x, y) in enumerate(zip(conv_a, conv_b)):
        if x != y:
            print('   first difference at', i, x, y)
            break
ok &= conv_a == conv_b
print('A/B', 'IDENTICAL' if ok else 'DIFFERS')
sys.exit(0 if ok else 1)
