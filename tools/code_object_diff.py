"""CPU tool: are the kernels of two builds the same device code?  For every kernel in the gfx950 code objects of two csrc
directories (each after `make`) it compares the function's bytes, its 64-byte kernel descriptor (less the entry offset, which
moves with the layout of the translation unit) and its resource note (VGPRs,
SGPRs, LDS, scratch, spills, kernarg size), and lists the kernels that appear, vanish or change translation unit.
python tools/code_object_diff.py PARENT_CSRC [NEW_CSRC]     (NEW_CSRC defaults to this tree's).  Exit status 1 on any difference
other than a move between translation units."""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

import yaml

LLVM = '/opt/rocm/lib/llvm/bin'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTE_KEYS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.group_segment_fixed_size',
             '.private_segment_fixed_size', '.kernarg_segment_size', '.max_flat_workgroup_size', '.wavefront_size',
             '.uses_dynamic_stack')


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def kernels(csrc):
    """{kernel name: (translation unit, sha1 of code + descriptor, note tuple, code bytes)}"""
    out = {}
    for obj in sorted(glob.glob(os.path.join(csrc, '*.o'))):
        with tempfile.TemporaryDirectory() as td:
            fat, co = os.path.join(td, 'fat.bin'), os.path.join(td, 'co.o')
            if subprocess.run([f'{LLVM}/llvm-objcopy', '--dump-section', f'.hip_fatbin={fat}', obj, os.path.join(td, 'x.o')],
                              capture_output=True).returncode != 0:
                continue                                         # host-only translation unit
            run(f'{LLVM}/clang-offload-bundler', '--unbundle', '--type=o', f'--input={fat}',
                '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', f'--output={co}')
            image = open(co, 'rb').read()
            note = run(f'{LLVM}/llvm-readelf', '--notes', co)
            sections = run(f'{LLVM}/llvm-readelf', '-S', '-W', co)
            symbols = run(f'{LLVM}/llvm-readelf', '--symbols', '-W', co)
        # [Nr] Name Type Address Off Size ...
        sec = {int(m[1]): (int(m[2], 16), int(m[3], 16))
               for m in re.finditer(r'^\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+[0-9a-f]+', sections, re.M)}
        sym = {}
        for line in symbols.splitlines():
            f = line.split()
            if len(f) == 8 and f[3] in ('FUNC', 'OBJECT') and f[6].isdigit():
                addr, off = sec[int(f[6])]
                start = int(f[1], 16) - addr + off
                sym[f[7]] = image[start:start + int(f[2], 0)]
        meta = yaml.safe_load(note.split('---', 1)[1].rsplit('...', 1)[0])
        for k in meta['amdhsa.kernels']:
            name = k['.name']
            code, kd = sym[name], sym[k['.symbol']]
            assert code and len(kd) == 64, name
            # (bytes 16 - 23 of the descriptor are the distance from it to the code: where the linker put the two, not what they are)
            assert name not in out, f'{name} in two translation units'
            out[name] = (os.path.basename(obj), hashlib.sha1(code + kd[:16] + kd[24:]).hexdigest(), tuple(k.get(n, 0) for n in NOTE_KEYS), len(code))
    return out


def main():
    parent = kernels(sys.argv[1])
    new = kernels(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'gen_adversarial_amd', 'csrc'))
    gone, born = sorted(set(parent) - set(new)), sorted(set(new) - set(parent))
    both = sorted(set(parent) & set(new))
    code = [n for n in both if parent[n][1] != new[n][1]]
    notes = [n for n in both if parent[n][2] != new[n][2]]
    moved = [n for n in both if parent[n][0] != new[n][0]]
    print(f'kernels: parent {len(parent)}, new {len(new)}; in both {len(both)}, vanished {len(gone)}, appeared {len(born)}')
    print(f'code bytes compared: {sum(parent[n][3] for n in both)} (parent) / {sum(new[n][3] for n in both)} (new)')
    print(f'function bytes or kernel descriptor differ: {len(code)}')
    print(f'resource notes differ ({", ".join(k[1:] for k in NOTE_KEYS)}): {len(notes)}')
    print(f'translation unit changed: {len(moved)}')
    for n in moved:
        print(f'  {run("c++filt", n).strip()}: {parent[n][0]} -> {new[n][0]}')
    for title, names in (('vanished', gone), ('appeared', born), ('code differs', code), ('notes differ', notes)):
        for n in names:
            print(f'  {title}: {run("c++filt", n).strip()[:160]}')
    per = {}
    for n in both:
        per[new[n][0]] = per.get(new[n][0], 0) + 1
    print('kernels per translation unit (new): ' + ', '.join(f'{o} {c}' for o, c in sorted(per.items())))
    return 1 if gone or born or code or notes else 0


if __name__ == '__main__':
    sys.exit(main())
