"""CPU tests of the channel bank (pddc_bank_*, include/perseus_ddc.h; k_fir_i8x_bank in csrc/ddc_fir_i8.hip): the entry
points check their arguments before they touch a device, refuse without one like every compute entry point, and the
bank's kernels are in the object under the build-time hazard check (no packed fp32, every result store padded)."""
import ctypes as C
import os
import subprocess
import sys

import pytest


def test_bank_entry_points_check_their_arguments(pkg):
    L = pkg.ddc_lib()
    fake = [C.c_void_p(1 << 20), C.c_void_p(2 << 20)]    # never dereferenced: the argument checks come first
    members = (C.c_void_p * 2)(*[f.value for f in fake])
    h = C.c_void_p()
    assert L.pddc_bank_create(None, 0, members, 2) == pkg.PDDC_EINVAL
    assert L.pddc_bank_create(C.byref(h), 0, None, 2) == pkg.PDDC_EINVAL
    assert L.pddc_bank_create(C.byref(h), 0, members, 0) == pkg.PDDC_EINVAL
    assert L.pddc_bank_create(C.byref(h), 0, members, 9) == pkg.PDDC_EINVAL          # PDDC_BANK_MAX = 8
    same = (C.c_void_p * 2)(fake[0].value, fake[0].value)
    assert L.pddc_bank_create(C.byref(h), 0, same, 2) == pkg.PDDC_EINVAL              # one pipeline twice
    nulls = (C.c_void_p * 2)(fake[0].value, None)
    assert L.pddc_bank_create(C.byref(h), 0, nulls, 2) == pkg.PDDC_EINVAL
    assert h.value is None
    n = (C.c_size_t * 2)()
    nb = C.c_int(7)
    assert L.pddc_bank_process(None, None, 8, None, None, n, C.byref(nb), None) == pkg.PDDC_EINVAL
    assert nb.value == 0
    mask, launches = C.c_uint(), C.c_int()
    assert L.pddc_bank_schedule(None, 8, C.byref(mask), C.byref(launches)) == pkg.PDDC_EINVAL
    assert L.pddc_bank_destroy(None) == pkg.PDDC_OK
    if L.pddc_device_count() == 0:
        # good arguments, no GPU: refused like every compute entry point
        assert L.pddc_bank_create(C.byref(h), 0, members, 2) == pkg.PDDC_ENODEV
        assert b"no CPU fallback" in L.pddc_last_error()
        assert h.value is None


def test_bank_kernels_are_under_the_hazard_check(pkg):
    """the built object passes csrc/check_hazard_pads.py, and the kernels it checked include the bank's instantiations for
    2 and 4 channels at both history lengths (the script itself fails when they are missing)"""
    obj = os.path.join(pkg.CSRC, "ddc_fir_i8.o")
    if not os.path.exists(obj):
        pkg.build()
    out = subprocess.run([sys.executable, os.path.join(pkg.CSRC, "check_hazard_pads.py"), obj, "--list"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    checked = [l.split() for l in out.stdout.splitlines() if l.startswith("checked: ")]
    banks = {(int(w[3]), int(w[5])) for w in checked if w[1] == "bank"}
    assert banks == {(32, 2), (32, 4), (64, 2), (64, 4)}, out.stdout[-2000:]
    assert any(w[1] == "layout" for w in checked)           # the existing forms are still checked too
    assert "no packed fp32" in out.stdout


def _disasm(kernels):
    """a disassembly listing in llvm-objdump's form: {symbol: [instructions]}"""
    out = []
    for i, (name, code) in enumerate(kernels.items()):
        out.append(f"{i * 4096:016x} <{name}>:")
        out += ["\t" + ins for ins in code]
    return "\n".join(out) + "\n"


def test_hazard_check_fails_without_the_bank_kernels(pkg, monkeypatch, capsys):
    """the script's own verdict on synthetic listings: an object without the bank's instantiations for 2 and 4 channels,
    or with a bank kernel whose result store is not padded, fails; with both present and padded it passes"""
    sys.path.insert(0, pkg.CSRC)
    try:
        import check_hazard_pads as chk
    finally:
        sys.path.pop(0)
    padded = ["v_mfma_i32_16x16x64_i8 v[0:3], v[4:7], v[8:11], v[0:3]", "global_store_dwordx2 v[2:3], v[4:5], off nt",
              "s_nop 1", "s_endpgm"]
    layout1 = "_ZN4pddc9k_fir_i8xILi64ELi2ELb0ELi1ELi8EEEvNS_10FirI8xArgsExi"
    bank = {n: f"_ZN4pddc14k_fir_i8x_bankILi64ELi{n}EEEvNS_10FirI8xBankExi" for n in (2, 4)}

    def verdict(kernels):
        monkeypatch.setattr(chk, "disassemble", lambda obj, arch, llvm: _disasm(kernels))
        rc = chk.main(["unused.o", "--list"])
        return rc, capsys.readouterr()

    rc, out = verdict({layout1: padded})
    assert rc == 1 and "k_fir_i8x_bank instantiation for 2 channels" in out.err and "for 4 channels" in out.err
    rc, out = verdict({layout1: padded, bank[2]: padded})
    assert rc == 1 and "for 4 channels" in out.err and "for 2 channels" not in out.err
    unpadded = ["global_store_dwordx2 v[2:3], v[4:5], off nt", "v_mov_b32_e32 v4, 0", "s_endpgm"]
    rc, out = verdict({layout1: padded, bank[2]: padded, bank[4]: unpadded})
    assert rc == 1 and "result store without its pad" in out.err and "k_fir_i8x_bankILi64ELi4E" in out.err
    packed = padded[:1] + ["v_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7]"] + padded[1:]
    rc, out = verdict({layout1: padded, bank[2]: packed, bank[4]: padded})
    assert rc == 1 and "packed fp32" in out.err
    rc, out = verdict({layout1: padded, bank[2]: padded, bank[4]: padded})
    assert rc == 0, out.err
    assert out.out.count("checked: bank") == 2 and "no packed fp32" in out.out


def test_bank_abi_is_declared(pkg):
    hdr = open(os.path.join(os.path.dirname(pkg.CSRC), "..", "include", "perseus_ddc.h")).read()
    for sym in ("pddc_bank_create", "pddc_bank_destroy", "pddc_bank_process", "pddc_bank_schedule"):
        assert sym + "(" in hdr
        assert hasattr(pkg.ddc_lib(), sym)
    assert "#define PDDC_BANK_MAX 8" in hdr
