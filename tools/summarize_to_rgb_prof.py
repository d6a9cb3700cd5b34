"""Per-kernel milliseconds and HBM bytes of a to_rgb_stack profile (tools/prof_to_rgb.py under rocprofv3).

    python tools/summarize_to_rgb_prof.py DIR [data ...]      (default data: exponential constant)

DIR holds kernel_trace_<data>.csv (rocprofv3 --kernel-trace) and counters_<data>_FETCH_SIZE.csv /
_WRITE_SIZE.csv (rocprofv3 --pmc, one counter per run; the counters count KiB).  Prints one
JSON line per data set: for the last call of the trace, every rgb_ kernel launch in order with its
milliseconds, and the bytes fetched / written by the launches of the counter run's last call.
"""
import csv
import json
import os
import sys


def short(name):
    for key in ('rgb_hist_kernel', 'rgb_select_kernel', 'rgb_compose_kernel'):
        if key in name:
            targs = name.split(key)[1].split('>')[0].lstrip('<')
            return '%s<%s>' % (key, targs)
    return None


def launches(path, value=None):
    out = []
    for row in csv.DictReader(open(path)):
        nm = short(row['Kernel_Name'])
        if nm is None or (value and row.get('Counter_Name') != value):
            continue
        out.append((int(row['Start_Timestamp']), nm, (int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1e6,
                    float(row['Counter_Value']) if value else None))
    out.sort()
    return out


def last_call(rows):
    """the launches from the last pass-0 histogram on"""
    first = max(i for i, r in enumerate(rows) if 'hist_kernel' in r[1] and 'true' in r[1])
    return rows[first:]


def main():
    d = sys.argv[1]
    for data in (sys.argv[2:] or ['exponential', 'constant']):
        tr = last_call(launches(os.path.join(d, 'kernel_trace_%s.csv' % data)))
        fe = last_call(launches(os.path.join(d, 'counters_%s_FETCH_SIZE.csv' % data), 'FETCH_SIZE'))
        wr = last_call(launches(os.path.join(d, 'counters_%s_WRITE_SIZE.csv' % data), 'WRITE_SIZE'))
        rows = []
        for i, (_, nm, ms, _) in enumerate(tr):
            rows.append(dict(kernel=nm, ms=round(ms, 4),
                             fetch_gb=round(fe[i][3] * 1024 / 1e9, 4) if i < len(fe) and fe[i][1] == nm else None,
                             write_gb=round(wr[i][3] * 1024 / 1e9, 4) if i < len(wr) and wr[i][1] == nm else None))
        print(json.dumps(dict(data=data, total_ms=round(sum(r['ms'] for r in rows), 4), launches=rows)))


if __name__ == '__main__':
    main()
