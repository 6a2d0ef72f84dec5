"""Per-kernel instruction statistics of a `hipcc -save-temps` assembly file (gfx950): VALU / v_mov / LDS / waits on lgkmcnt(0), registers, scratch.
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I include -save-temps -o /tmp/isa/lib.so kmerdb_amd/csrc/kdb_engine.hip
    python tools/isa_stats.py /tmp/isa/kdb_engine-hip-amdgcn-amd-amdhsa-gfx950.s [substring ...]
    python tools/isa_stats.py --diff A.s B.s          (are the kernels of two builds the same, name for name and line for line?)
A returning LDS atomic followed at once by `s_waitcnt lgkmcnt(0)`, or dozens of v_mov per atomic, is how round 4 found the histogram adds
the compiler had serialised."""
import re
import subprocess
import sys


def kernel_bodies(path):
    """-> {mangled kernel name: the lines behind its label}, for the functions that end a program"""
    funcs, cur = {}, None
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif cur is not None:
            funcs[cur].append(line.rstrip("\n"))
    return {n: b for n, b in funcs.items() if any('s_endpgm' in x for x in b)}


def kernel_stats(path):
    """-> {demangled kernel name: {insts, valu, v_mov, salu, ds, ds_rtn_atomics, vmem, waits_lgkmcnt0, barriers, vgprs, scratch, occupancy, lds}}"""
    funcs = kernel_bodies(path)
    names = list(funcs)
    dem = subprocess.run(['c++filt'], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for n, d in zip(names, dem):
        b = funcs[n]
        ins = [x.strip() for x in b if x.startswith('\t') and not x.strip().startswith(('.', ';'))]
        cnt = lambda p: sum(1 for x in ins if x.startswith(p))          # noqa: E731
        info = {k: next((x.split(':')[1].strip() for x in b if ('; ' + k + ':') in x), '?') for k in ('NumVgprs', 'ScratchSize', 'Occupancy', 'LDSByteSize')}
        num = lambda v: int(v.split(' ')[0]) if v.split(' ')[0].isdigit() else None          # noqa: E731
        out[d] = {"insts": len(ins), "valu": cnt('v_'), "v_mov": cnt('v_mov'), "salu": cnt('s_') - cnt('s_waitcnt'), "ds": cnt('ds_'),
                  "ds_rtn_atomics": sum(1 for x in ins if x.startswith('ds_') and '_rtn_' in x), "vmem": cnt('global_') + cnt('buffer_') + cnt('flat_'),
                  "waits_lgkmcnt0": sum(1 for x in ins if x.startswith('s_waitcnt') and 'lgkmcnt(0)' in x), "barriers": cnt('s_barrier'),
                  "vgprs": num(info['NumVgprs']), "scratch": num(info['ScratchSize']), "occupancy": num(info['Occupancy']), "lds": num(info['LDSByteSize'])}
    return out


def diff(path_a, path_b):
    """Compare two builds kernel by kernel.  A kernel's local labels carry its position in the file (.LBB<n>_, BB<n>_ in comments, .Lfunc_end<n>): the position is
    masked, so that kernels emitted in another order still compare equal; lines that name the per-build __hip_cuid_ symbol are left out."""
    def norm(body):
        end = body.index("; Kernel info:")          # the kernel ends with this block of comments: behind it the next function is announced
        while end < len(body) and body[end].startswith(";"):
            end += 1
        return [re.sub(r'(BB|Lfunc_end|Lfunc_begin)\d+', r'\1#', x) for x in body[:end] if '__hip_cuid_' not in x]
    a, b = kernel_bodies(path_a), kernel_bodies(path_b)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = [n for n in a if n in b and norm(a[n]) != norm(b[n])]
    print("kernels: %d in A, %d in B; only in A: %d, only in B: %d; in both but different: %d" % (len(a), len(b), len(only_a), len(only_b), len(differ)))
    for tag, names in (("only in A", only_a), ("only in B", only_b), ("different", differ)):
        for n in names:
            print("  %s: %s" % (tag, n[:200]))
    return 1 if only_a or only_b or differ else 0


def main():
    if sys.argv[1] == "--diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    path, pats = sys.argv[1], sys.argv[2:]
    for d, v in kernel_stats(path).items():
        if pats and not any(p in d for p in pats):
            continue
        print("%s\n    insts %d  valu %d  v_mov %d  salu %d  ds %d  ds_rtn_atomics %d  vmem %d  waits_lgkmcnt0 %d  barriers %d | vgprs %s scratch %s occ %s lds %s" % (
            d[:150], v["insts"], v["valu"], v["v_mov"], v["salu"], v["ds"], v["ds_rtn_atomics"], v["vmem"], v["waits_lgkmcnt0"], v["barriers"],
            v["vgprs"], v["scratch"], v["occupancy"], v["lds"]))


if __name__ == "__main__":
    main()
