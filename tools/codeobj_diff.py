#!/usr/bin/env python
"""tools/codeobj_diff.py -- compare the gfx950 code objects of two builds, kernel by kernel.  No GPU.

    python tools/codeobj_diff.py PARENT_OBJDIR BRANCH_OBJDIR [unit ...]

The two directories hold the object files of `python -m nd_amd.build` (nd_amd/csrc/_build) of two trees; `unit`
narrows the comparison to some translation units (omnibus, omnibus_c3, ...).  For each unit the device code
object is taken out of the object file (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler
--unbundle), disassembled (llvm-objdump -d; addresses and encodings dropped, the pc-relative literal behind
s_getpc_b64 masked, the zero padding between two symbols left out: both depend on the order of the kernels) and split per symbol; the resource figures are read from the code object's
metadata (llvm-readelf --notes).  Reported: the kernels removed, added, differing in text, and differing in any
resource figure.  Exit status 1 if anything differs.
"""
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
FIGURES = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size',
           '.vgpr_spill_count', '.sgpr_spill_count', '.kernarg_segment_size', '.max_flat_workgroup_size')


def _tool(name):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    for d in (os.path.join(os.path.dirname(os.path.realpath(hipcc)), '..', 'lib', 'llvm', 'bin'), '/opt/rocm/lib/llvm/bin'):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    found = shutil.which(name)
    if not found:
        raise RuntimeError('%s not found' % name)
    return found


def code_object(obj, tmp):
    """-> path of the gfx950 code object inside the object file `obj`, None for a host-only unit"""
    fat = os.path.join(tmp, 'fatbin')
    co = os.path.join(tmp, 'gfx950.co')
    sections = subprocess.run([_tool('llvm-readelf'), '-S', obj], check=True, stdout=subprocess.PIPE, text=True).stdout
    if '.hip_fatbin' not in sections:
        return None
    subprocess.check_call([_tool('llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, obj, os.path.join(tmp, 'rest.o')])
    subprocess.check_call([_tool('clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + TARGET,
                           '--input=' + fat, '--output=' + co])
    return co


def kernels(co):
    """-> {symbol: {figure: value}} from the code object's metadata note"""
    notes = subprocess.run([_tool('llvm-readelf'), '--notes', co], check=True, stdout=subprocess.PIPE, text=True).stdout
    out, cur = {}, None
    for ln in notes.splitlines():
        m = re.match(r'  (- |  )(\.[a-z_]+):\s*(\S+)\s*$', ln)      # a kernel record's own keys, not its arguments'
        if not m:
            continue
        if m.group(1) == '- ':
            cur = {}
        key, val = m.group(2), m.group(3)
        if cur is None:
            continue
        if key == '.symbol':
            out[val[:-3] if val.endswith('.kd') else val] = cur
        elif key in FIGURES:
            cur[key] = int(val)
    return out


def disassembly(co):
    """-> {symbol: [instruction lines without addresses]}"""
    text = subprocess.run([_tool('llvm-objdump'), '-d', '--no-show-raw-insn', co], check=True, stdout=subprocess.PIPE,
                          text=True).stdout
    out, cur, after_getpc = {}, None, 0
    for ln in text.splitlines():
        m = re.match(r'[0-9a-f]+ <(.+)>:$', ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not ln.strip() or ln.strip() == '...':      # ("...": zero padding up to the next symbol)
            continue
        ins = re.sub(r'\s*//.*$', '', ln).strip()                     # (the address and the encoding)
        if after_getpc and re.match(r's_addc?_u32', ins):
            ins = re.sub(r',\s*\S+$', ', <pcrel>', ins)                # the literal depends on where the kernel lies
            after_getpc -= 1
        else:
            after_getpc = 0
        if ins.startswith('s_getpc_b64'):
            after_getpc = 2
        cur.append(ins)
    return out


def unit(obj):
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(obj, tmp)
        return (kernels(co), disassembly(co)) if co else ({}, {})


def compare(name, a_obj, b_obj, out):
    (ka, da), (kb, db) = unit(a_obj), unit(b_obj)
    removed, added = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    text, res = [], []
    for sym in sorted(set(ka) & set(kb)):
        if da.get(sym) != db.get(sym):
            la, lb = da.get(sym, []), db.get(sym, [])
            n = sum(1 for d in difflib.unified_diff(la, lb, lineterm='', n=0) if d[:1] in '+-' and d[:3] not in ('+++', '---'))
            text.append('    differs: %s  (%d lines differ; %d -> %d)' % (sym, n, len(la), len(lb)))
        moved = [(f, ka[sym].get(f), kb[sym].get(f)) for f in FIGURES if ka[sym].get(f) != kb[sym].get(f)]
        if moved:
            res.append('    resource: %s %s' % (sym, moved))
    out.append('%s.hip  kernels parent %d branch %d removed %d  added %d  differing in text %d  in a resource figure %d'
               % (name, len(ka), len(kb), len(removed), len(added), len(text), len(res)))
    out.extend('    removed: ' + s for s in removed)
    out.extend('    added: ' + s for s in added)
    out.extend(text)
    out.extend(res)
    return bool(removed or added or text or res)


def main(argv):
    if len(argv) < 3:
        sys.stderr.write(__doc__)
        return 2
    a_dir, b_dir, only = argv[1], argv[2], argv[3:]
    names = sorted(f[:-2] for f in os.listdir(a_dir) if f.endswith('.o'))
    names_b = sorted(f[:-2] for f in os.listdir(b_dir) if f.endswith('.o'))
    out, differs = [], False
    if not only and names != names_b:
        out.append('translation units only in one build: %s' % sorted(set(names) ^ set(names_b)))
        differs = True
    for name in (only or sorted(set(names) & set(names_b))):
        differs = compare(name, os.path.join(a_dir, name + '.o'), os.path.join(b_dir, name + '.o'), out) or differs
    print('\n'.join(out))
    return 1 if differs else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
