"""CPU: static audit of the one-tile bf16 GEMM's ISA (csrc/gemm_bf16_kernel.hpp, every instance in gemm_bf16.hip).

The LayerNorm-aware kernels (the fused Q/K/V + attention among them) load their rows' statistics by inline asm, ahead of the
operand DMA, and retire them with a hand-counted `s_waitcnt vmcnt` that carries a `; STATRETIRE <registers>` comment.  The
compiler does not know those registers are in flight: an instruction it places between a load and its retiring wait that
reads one of them (a live-range copy, a spill) uses garbage on some launches only.  Two waits in the arms of a
`K >= STA * 64` branch once made it copy the registers in front of the branch (K = 128: a whole tile's statistics wrong, now
and then).  The listing must show no such instruction, no scratch, and a retiring wait for every asm load."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]


def _regs(tok):
    out = []
    for m in re.finditer(r"v\[(\d+):(\d+)\]|\bv(\d+)\b", tok):
        out += list(range(int(m.group(1)), int(m.group(2)) + 1)) if m.group(1) else [int(m.group(3))]
    return out


def _instructions(lines):
    """(index, op, operands, in_asm, line) of a function's instructions, labels as ('label', name)"""
    out, inasm = [], False
    for i, l in enumerate(lines):
        if "ASMSTART" in l or "ASMEND" in l:
            inasm = "ASMSTART" in l
            continue
        c = l.split(";")[0].strip()
        if re.match(r"^\.?L?BB[\w.]*:$|^\.LBB\w*:$", c):
            out.append(("label", c[:-1]))
            continue
        if not c or c.startswith("."):
            if "STATRETIRE" in l:
                out.append((i, "retire", l.split("STATRETIRE")[1], inasm, l))
            continue
        op, _, rest = c.partition(" ")
        if "STATRETIRE" in l:
            out.append((i, "retire", l.split("STATRETIRE")[1], inasm, l))
            continue
        out.append((i, op, rest, inasm, c))
    return out


def _audit_function(name, lines, problems):
    """forward dataflow over the basic blocks: the set of asm-load destinations that may be in flight"""
    ins = _instructions(lines)
    blocks, cur, labels = [], [], {}
    for x in ins:
        if x[0] == "label":
            if cur:
                blocks.append(cur)
            cur = []
            labels[x[1]] = len(blocks)
            continue
        cur.append(x)
        if x[1].startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc")):
            blocks.append(cur)
            cur = []
    if cur:
        blocks.append(cur)
    succ = []
    for b, blk in enumerate(blocks):
        last = blk[-1][1] if blk else ""
        tgt = blk[-1][2].strip() if blk else ""
        s = []
        if last.startswith(("s_branch", "s_cbranch")):
            s.append(labels.get(tgt))
        if not last.startswith(("s_branch", "s_endpgm", "s_setpc")):
            s.append(b + 1 if b + 1 < len(blocks) else None)
        succ.append([x for x in s if x is not None])
    state_in = [None] * len(blocks)
    state_in[0] = frozenset()
    work, loads, seen = [0], 0, set()
    while work:
        b = work.pop()
        pend = set(state_in[b])
        for (i, op, rest, inasm, text) in blocks[b]:
            if op == "retire":
                pend -= set(_regs(rest))
                continue
            if "scratch_" in op:
                seen.add((i, "scratch access: " + text))
            if inasm and op.startswith("global_load") and " lds" not in rest:
                loads += 1
                pend |= set(_regs(rest.split(",")[0]))
                continue
            if op.startswith("s_"):
                continue
            # a read of an in-flight destination is the hazard; a plain write redefines the register (the compiler only does that
            # where the loaded value is dead: on paths that never issued the loads, e.g. LayerNorm-free calls)
            first, _, others = rest.partition(",")
            writes = op.startswith(("v_", "ds_read", "global_load", "buffer_load")) and not op.startswith("v_cmp") and bool(_regs(first))
            uses = _regs(others) + (_regs(first) if not writes or "mac" in op or "sdwa" in op or "dpp" in op else [])
            hit = set(uses) & pend
            if hit:
                seen.add((i, f"reads in-flight statistics register(s) v{sorted(hit)}: " + text))
            if writes:
                pend -= set(_regs(first))
        for t in succ[b]:
            new = frozenset(pend) | (state_in[t] or frozenset())
            if state_in[t] is None or new != state_in[t]:
                state_in[t] = new
                work.append(t)
        if not succ[b] and pend and blocks[b] and blocks[b][-1][1] == "s_endpgm":
            seen.add((-1, f"asm-load destination(s) v{sorted(pend)} in flight at s_endpgm"))
    problems += [(name, i, t) for i, t in sorted(seen)]
    return loads


def audit(asm_text: str) -> list:
    S = asm_text.split("\n")
    problems = []
    starts = [i for i, l in enumerate(S) if re.match(r"^_ZN\d+_GLOBAL__N_1\d+gemm_bf16_kernel.*:", l)]
    assert starts, "no gemm_bf16_kernel in the listing"
    loads = 0
    for st in starts:
        en = st
        while not S[en].startswith(".Lfunc_end"):
            en += 1
        loads += _audit_function(S[st].split(":")[0], S[st + 1:en], problems)
    assert loads, "no inline-asm statistics loads found: the audit would pass vacuously"
    return problems


def _listing(tmp: Path) -> str:
    sys.path.insert(0, str(REPO))
    from ultrafnd_git_amd.build import ARCH
    src = REPO / "ultrafnd_git_amd" / "csrc" / "gemm_bf16.hip"
    subprocess.run(["/opt/rocm/bin/hipcc", f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", "-I", str(REPO / "include"),
                    "-S", "--offload-device-only", str(src), "-o", str(tmp / "gemm.s")], check=True, capture_output=True)
    return (tmp / "gemm.s").read_text()


def test_gemm_isa_reads_no_statistics_register_before_its_wait():
    with tempfile.TemporaryDirectory() as t:
        problems = audit(_listing(Path(t)))
    assert not problems, problems[:5]


def test_the_audit_sees_a_planted_hazard():
    good = """_ZN12_GLOBAL__N_116gemm_bf16_kernelILi9EEEvNS_8GemmArgsE:
\t;;#ASMSTART
\tglobal_load_dwordx4 v[10:13], v[2:3], off
\t;;#ASMEND
\tglobal_load_lds_dwordx4 v[4:5], off
\tv_add_f32_e32 v20, v21, v22
\t;;#ASMSTART
\ts_waitcnt vmcnt(18) ; STATRETIRE v[10:13]
\t;;#ASMEND
\tv_add_f32_e32 v20, v10, v22
.Lfunc_end0:
"""
    assert audit(good) == []
    assert audit(good.replace("v_add_f32_e32 v20, v21, v22", "v_mov_b64_e32 v[30:31], v[12:13]"))
    assert audit(good.replace("; STATRETIRE v[10:13]", ""))
    assert audit(good.replace("v_add_f32_e32 v20, v21, v22", "global_store_dwordx4 v[30:31], v[10:13], off"))
    assert audit(good.replace("v_add_f32_e32 v20, v21, v22", "v_fmac_f32_e32 v11, v21, v22"))
