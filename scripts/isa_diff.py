"""Per-kernel diff of the gfx950 instruction streams of two builds of libvidtok_amd.so (no GPU needed).

    python scripts/isa_diff.py OLD.so NEW.so [--show N]

Extracts the gfx950 code object of each library (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler), disassembles it
(llvm-objdump -d, no addresses, no encodings), splits it per function and compares the kernels of OLD one by one with their
counterparts in NEW.  Instruction operands that encode a position in the code object (PC-relative offsets of global symbols after
s_getpc_b64) are masked, so a kernel that moved in the file still compares equal.  Pairing: a kernel keeps its mangled name, except
that conv_igemm_glds_kernel grew a last template argument ACT (0 = no activation) -- OLD's <..., SCHED> is NEW's <..., SCHED, 0>.
Prints one line per changed / missing kernel and a one-line verdict; exit status 1 if any kernel of OLD changed or disappeared.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM_BIN = "/opt/rocm/lib/llvm/bin"
ACT0_SUFFIX = ("ELi0EEEvNS_8ConvArgsE", "EEEvNS_8ConvArgsE")     # NEW's trailing ACT = 0 argument -> OLD's name


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def disassemble(so):
    """disassembly of every gfx950 code object of the library: the .hip_fatbin section holds one offload bundle per translation unit"""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([f"{LLVM_BIN}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", so, os.path.join(d, "discard.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        text = []
        for i, s0 in enumerate(starts):
            part, dev = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"b{i}.co")
            with open(part, "wb") as f:
                f.write(blob[s0: starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.check_call([f"{LLVM_BIN}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}",
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={dev}"])
            text.append(subprocess.check_output([f"{LLVM_BIN}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", dev], text=True))
        return "\n".join(text)


def functions(text):
    """{symbol: [normalised instruction lines]}"""
    out, cur = {}, None
    head = re.compile(r"^(?:[0-9a-f]+ )?<(.+)>:$")
    for line in text.splitlines():
        m = head.match(line.strip())
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if "file format" in line or line.startswith("Disassembly of section"):
            cur = None                                     # the next code object's header
        if cur is None:
            continue
        ins = line.split("//")[0].strip()
        if not ins or ins == "...":                        # objdump's mark for the zero fill behind a code object's LAST function: which one
            continue                                       # that is follows the order of instantiation in the host code, not the kernel
        ins = re.sub(r"<[^>]*>", "", ins).strip()          # branch target annotations (symbol + offset)
        out[cur].append(ins)
    for name, ins in out.items():                          # operands of the s_add/s_addc pair after s_getpc_b64: a symbol's distance
        for i, s in enumerate(ins):
            if s.startswith("s_getpc_b64"):
                for k in range(i + 1, min(i + 4, len(ins))):
                    if ins[k].startswith(("s_add_u32", "s_addc_u32", "s_add_co_u32", "s_add_co_ci_u32")):
                        ins[k] = re.sub(r"0x[0-9a-f]+|-?\b\d+\b$", "<pcrel>", ins[k])
    return out


def main(argv):
    old_so, new_so = argv[1], argv[2]
    show = int(argv[argv.index("--show") + 1]) if "--show" in argv else 0
    old, new = functions(disassemble(old_so)), functions(disassemble(new_so))
    new_by_old_name = {}
    for n in new:
        k = n[: -len(ACT0_SUFFIX[0])] + ACT0_SUFFIX[1] if "conv_igemm_glds_kernel" in n and n.endswith(ACT0_SUFFIX[0]) else n
        new_by_old_name[k] = n
    for n in new:                  # both builds after the ACT argument: a kernel pairs with its own name first
        if n in old:
            new_by_old_name[n] = n
    same, changed, missing, renamed = 0, [], [], 0
    for name, ins in sorted(old.items()):
        if name not in new_by_old_name:
            missing.append(name)
            continue
        nn = new_by_old_name[name]
        renamed += nn != name
        if new[nn] == ins:
            same += 1
        else:
            changed.append(name)
            print(f"CHANGED {name}: {len(ins)} -> {len(new[nn])} instructions")
            if show:
                import difflib
                for ln in list(difflib.unified_diff(ins, new[nn], lineterm="", n=1))[:show]:
                    print("   ", ln)
    for name in missing:
        print(f"MISSING {name}")
    added = len(new) - (len(old) - len(missing))
    verdict = "IDENTICAL" if not changed and not missing else "DIFFERENT"
    print(f"isa_diff: {verdict}: {same} of {len(old)} functions of the old library have the same gfx950 instruction stream "
          f"({renamed} paired across the added ACT template argument), {len(changed)} changed, {len(missing)} missing; "
          f"{added} functions are new")
    return 0 if verdict == "IDENTICAL" else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
