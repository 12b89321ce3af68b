"""tools/kernel_text_diff.py on two tiny made-up listings in the form `hipcc -save-temps=obj` leaves: the same kernels in another order
and with other label numbers are equal; one changed instruction names its kernel and fails; a kernel missing on one side fails."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernel(name, fn, imm):
    return (f"\t.globl\t{name}\n\t.p2align\t8\n\t.type\t{name},@function\n"
            f"{name}:                                 ; @{name}\n; %bb.0:\n"
            f"\ts_load_dword s0, s[4:5], 0x{imm:x}\n\ts_cbranch_scc1 .LBB{fn}_2              ; comment {fn}\n"
            f"; %bb.1:                                ; %in.qs_body{fn}\n\tv_add_u32_e32 v0, s0, v0\n.LBB{fn}_2:\n.Ltmp{fn * 3}:\n\ts_endpgm\n"
            f"\t.section\t.rodata,\"a\",@progbits\n.Lfunc_end{fn}:\n\t.size\t{name}, .Lfunc_end{fn}-{name}\n; -- End function\n"
            f"\t.set {name}.num_vgpr, {fn}\n")


A, B = "_ZN3fpx1aILi8ELb0EEEvNS_4ArgsE", "_ZN3fpx1bILi16ELb1EEEvNS_4ArgsE"


def _diff(tmp_path, old, new):
    (tmp_path / "old.s").write_text(old)
    (tmp_path / "new.s").write_text(new)
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_text_diff.py"), str(tmp_path / "old.s"), str(tmp_path / "new.s")],
                          capture_output=True, text=True, timeout=60)


def test_another_order_and_other_label_numbers_are_equal(tmp_path):
    r = _diff(tmp_path, _kernel(A, 0, 0x10) + _kernel(B, 1, 0x20), _kernel(B, 7, 0x20) + _kernel(A, 12, 0x10))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "kernels: 2 old, 2 new; names the same set" in r.stdout and "bodies that differ: 0" in r.stdout and "order: differs" in r.stdout


def test_one_changed_instruction_names_its_kernel(tmp_path):
    r = _diff(tmp_path, _kernel(A, 0, 0x10) + _kernel(B, 1, 0x20), _kernel(A, 0, 0x10) + _kernel(B, 1, 0x24))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "bodies that differ: 1" in r.stdout and "differs: " + B in r.stdout and "differs: " + A not in r.stdout
    assert "order: the same" in r.stdout


def test_a_missing_kernel_fails(tmp_path):
    r = _diff(tmp_path, _kernel(A, 0, 0x10) + _kernel(B, 1, 0x20), _kernel(A, 0, 0x10))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "names DIFFER" in r.stdout and "only in old: " + B in r.stdout
