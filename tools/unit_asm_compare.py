"""Is the device code of a set of translation units that of one earlier translation unit, function by function?

    hipcc <pgtg_amd.build.FLAGS without -shared> --cuda-device-only -S -o old.s  <the old source>
    hipcc <the same>                                               -S -o unitN.s <each new source>
    python tools/unit_asm_compare.py old.s unit1.s unit2.s ...

A function's text runs from its "Begin function" line to the next one: its instructions, its kernel descriptor
(.amdhsa_kernel block), its .set resource symbols and the "Kernel info" / "Function info" comment block with the
registers, LDS, scratch and occupancy.  Local labels carry the function's index in its file (.LBB12_3,
.Lfunc_end12), which moves when functions move between files: the index is dropped before the texts are compared,
runs of blanks count as one, and the section directive that opens the next function is left out.
Prints one line per function of old.s and a resource table per new unit; exit status 1 unless every function of
old.s is in exactly one unit with the same text and the units hold no others."""
import re
import sys

BEGIN = re.compile(r"; -- Begin function (\S+)")
# what follows the last function of a file
TAIL = re.compile(r"^\t\.(?:p2alignl|amdgpu_metadata)|^\t\.section\t\.AMDGPU\.gpr_maximums|^\t\.type\t__hip_cuid", re.M)
LOCAL = re.compile(r"(\.L(?:BB|func_end|func_begin|JTI|tmp|CPI)|\bBB)\d+")  # (BB12_3: the loop comments)
NEXT_SECTION = re.compile(r"\t\.(?:text|section\t\.text\S*)\n\Z")  # the section of the function that follows
FIELDS = ["NumVgprs", "NumAgprs", "TotalNumSgprs", "LDSByteSize", "ScratchSize", "Occupancy"]


def functions(path):
    text = open(path).read()
    marks = list(BEGIN.finditer(text))
    out = {}
    for m, nxt in zip(marks, marks[1:] + [None]):
        start = text.rfind("\n", 0, m.start()) + 1
        end = text.rfind("\n", 0, nxt.start()) + 1 if nxt else len(text)
        body = text[start:end]
        if not nxt and (t := TAIL.search(body)):
            body = body[:t.start()]
        assert m.group(1) not in out, f"{path}: {m.group(1)} twice"
        body = LOCAL.sub(lambda l: l.group(1), NEXT_SECTION.sub("", body))
        out[m.group(1)] = re.sub(r"[ \t]+", " ", body)  # (comments are aligned in columns: a shorter label shifts them)
    return out


def resources(body):
    if ".amdhsa_kernel" not in body:
        return None
    return [re.search(rf"; {f}: (\d+)", body).group(1) for f in FIELDS]


def main(old_path, *unit_paths):
    old = functions(old_path)
    units = {p: functions(p) for p in unit_paths}
    bad = 0
    for name, body in old.items():
        homes = [p for p, fs in units.items() if name in fs]
        if len(homes) != 1:
            verdict = "MISSING" if not homes else "IN " + " AND ".join(homes)
        else:
            verdict = "same" if units[homes[0]][name] == body else "DIFFERS"
        bad += verdict != "same"
        print(f"{verdict:8s} {'kernel  ' if resources(body) else 'function'} {homes[0] if len(homes) == 1 else '-'}  {name}")
    for p, fs in units.items():
        for name in fs:
            if name not in old:
                bad += 1
                print(f"NEW      {p}  {name}")
    for p, fs in {old_path: old, **units}.items():
        print(f"\n{p}: kernels\n" + " ".join(f"{f:>13s}" for f in FIELDS) + "  name")
        for name, body in fs.items():
            if r := resources(body):
                print(" ".join(f"{v:>13s}" for v in r) + "  " + name)
    print(f"\n{len(old)} functions in {old_path}, {bad} not the same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
