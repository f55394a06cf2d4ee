"""quic-test_amd/csrc/tools/asm_diff.py on hand-written snippets: functions that differ only in
comments and local label numbers are the same; a changed instruction and a missing function are
reported, with a non-zero exit status."""
import subprocess
import sys
from pathlib import Path

TOOL = Path(__file__).resolve().parent.parent / "quic-test_amd" / "csrc" / "tools" / "asm_diff.py"


def _func(name, index, body, vgprs=8):
    return (f"\t.globl\t{name}\n\t.type\t{name},@function\n{name}: ; @{name}\n; %bb.0:\n{body}"
            f".Lfunc_end{index}:\n\t.size\t{name}, .Lfunc_end{index}-{name}\n"
            f"\t.section\t.rodata\n\t.amdhsa_kernel {name}\n\t\t.amdhsa_next_free_vgpr {vgprs}\n\t.end_amdhsa_kernel\n\t.text\n")


def _loop(index, first, op="v_xor_b32_e32", note="Inner Loop Header"):
    return (f"\ts_load_dword s2, s[0:1], 0x0 ; a comment\n.LBB{index}_{first}: ; ={note}\n"
            f"\t{op} v1, v1, v2\n\ts_cbranch_scc1 .LBB{index}_{first}\n; %bb.{first + 1}:\n"
            f"\ts_cbranch_scc0 .LBB{index}_{first + 3}\n.LBB{index}_{first + 3}:\n\ts_endpgm\n")


def _run(tmp_path, a, b):
    (tmp_path / "a.s").write_text(a)
    (tmp_path / "b.s").write_text(b)
    return subprocess.run([sys.executable, str(TOOL), "a.s", "b.s"], cwd=tmp_path, capture_output=True, text=True)


def test_comments_and_label_numbers_do_not_count(tmp_path):
    a = _func("_Z3fooPi", 0, _loop(0, 1)) + _func("_Z3barPi", 1, _loop(1, 2))
    # the other order, other label numbers, other comments
    b = _func("_Z3barPi", 0, _loop(0, 7, note="another note")) + _func("_Z3fooPi", 1, _loop(1, 4, note="x"))
    res = _run(tmp_path, a, b)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "2 functions on both sides, 0 differ; 0 only in a.s, 0 only in b.s" in res.stdout
    assert "differs" not in res.stdout


def test_changed_instruction_and_missing_function(tmp_path):
    a = _func("_Z3fooPi", 0, _loop(0, 1)) + _func("_Z3barPi", 1, _loop(1, 2)) + _func("_Z3bazPi", 2, _loop(2, 1))
    b = _func("_Z3fooPi", 0, _loop(0, 1, op="v_or_b32_e32") + "\ts_nop 0\n") + _func("_Z3barPi", 1, _loop(1, 2))
    res = _run(tmp_path, a, b)
    assert res.returncode == 1, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    differs = [ln for ln in lines if ln.startswith("differs")]
    assert len(differs) == 1 and ("foo(int*)" in differs[0] or "_Z3fooPi" in differs[0])
    counts = differs[0].split()[1:3]
    assert int(counts[1]) == int(counts[0]) + 1                    # both line counts, b one longer
    assert any(ln.startswith("only in a.s:") and "baz" in ln for ln in lines)
    assert "2 functions on both sides, 1 differ; 1 only in a.s, 0 only in b.s" in lines[-1]
    # the other way round: the function is on b's side only
    res = _run(tmp_path, b, a)
    assert res.returncode == 1 and "1 differ; 0 only in a.s, 1 only in b.s" in res.stdout


def test_a_changed_register_budget_counts(tmp_path):
    """The kernel descriptor travels with its function: same instructions, another VGPR count."""
    res = _run(tmp_path, _func("_Z3fooPi", 0, _loop(0, 1)), _func("_Z3fooPi", 0, _loop(0, 1), vgprs=16))
    assert res.returncode == 1 and "1 differ" in res.stdout
