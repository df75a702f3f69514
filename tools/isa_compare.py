#!/usr/bin/env python3
"""Compare the device code of two builds of the render kernels, instance by instance, symbol names aside.

    hipcc <Makefile FLAGS KFLAGS> --cuda-device-only -S -o old/srt_kernels.s srt_kernels.hip   (the parent commit)
    hipcc <Makefile FLAGS KFLAGS> --cuda-device-only -S -o new/srt_kernels.s srt_kernels.hip   (this tree)
    python tools/isa_compare.py old/srt_kernels.s new/srt_kernels.s

Every kernel of the old listing must be in the new one under its name with `Lb0E` (a defaulted trailing `false`
template argument, such as MOMENTS or DIRECT) appended to its template arguments -- whatever its parameter types are then
spelled as -- or under its old name; its instructions and its
descriptor (registers, scratch, LDS, argument size) must be identical once label numbers and the kernel's own name are
normalised.  Kernels only in the new listing are listed with their register counts and scratch size.

The whole check, every kernel source against the parent commit (FLAGS, KFLAGS: the values in csrc/Makefile):

    git archive HEAD sexy-raytracer_amd/csrc include | tar -x -C old          (a checkout of the parent)
    for d in old .; do mkdir -p $d/asm; for f in $d/sexy-raytracer_amd/csrc/*.hip; do
      (cd $d/sexy-raytracer_amd/csrc && hipcc $FLAGS $KFLAGS --cuda-device-only -S -o - $(basename $f)) \
        > $d/asm/$(basename $f .hip).s; done; done
    for s in old/asm/*.s; do echo "== $(basename $s .s)"; python tools/isa_compare.py $s asm/$(basename $s); done"""
import re
import sys

FUNC = re.compile(r"^(_Z\S+):\s*(?:;.*)?$")


def kernels(path):
    """{mangled name: [normalised lines of its body]} for every kernel entry in an assembly listing."""
    out, name, body = {}, None, []
    for line in open(path):
        m = FUNC.match(line.rstrip("\n"))
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            s = line.split(";")[0].rstrip()
            if not s:
                continue
            s = s.replace(name, "<K>")
            s = re.sub(r"\.L(BB|tmp|func_end)\d+(_\d+)?", r".L\1", s)
            body.append(s)
    return out


def meta(path):
    """{kernel name: {key: value}} from the amdhsa kernel descriptors (register counts, scratch, LDS)."""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is not None:
            if ".end_amdhsa_kernel" in line:
                cur = None
                continue
            m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size|group_segment_fixed_size|accum_offset)\s+(\S+)", line)
            if m:
                cur[m.group(1)] = m.group(2)
    return out


def new_name(old, new=()):
    m = re.match(r"(.*I(?:L[bi]\d+E)+)(EE?v)(.*)", old)  # EEv: a kernel in a namespace (a nested name)
    if not m:
        return old
    name = m.group(1) + "Lb0E" + m.group(2)
    # the parameter types may now depend on the new argument (srt_paths_kernel<MODE, DIRECT>: conditional_t<DIRECT, ...>)
    found = [n for n in new if n.startswith(name)]
    return found[0] if len(found) == 1 else name + m.group(3)


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    mo, mn = meta(old_path), meta(new_path)
    bad, matched = 0, set()
    for k, body in sorted(old.items()):
        n = new_name(k, new) if new_name(k, new) in new else k
        if n not in new:
            print("MISSING  %s" % k)
            bad += 1
            continue
        matched.add(n)
        same = new[n] == body and mo.get(k) == mn.get(n)
        print("%s %s (%d lines) %s" % ("same    " if same else "CHANGED ", k, len(body), mn.get(n)))
        bad += 0 if same else 1
    for n in sorted(set(new) - matched):
        print("new      %s %s" % (n, mn.get(n)))
    print("%d kernels compared, %d differ or are missing" % (len(old), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
