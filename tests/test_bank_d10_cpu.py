"""CPU tests of the channel bank's decimate-by-10 form (k_fir_i8x_bank<64, 2, 10> in csrc/ddc_fir_i8.hip, pddc_bank_* in
include/perseus_ddc.h): the built object holds it under the build-time hazard check, the check names each bank kernel's
decimation, and the header documents which members pair up."""
import os
import re
import subprocess
import sys


def _listing(pkg):
    obj = os.path.join(pkg.CSRC, "ddc_fir_i8.o")
    if not os.path.exists(obj):
        pkg.build()
    out = subprocess.run([sys.executable, os.path.join(pkg.CSRC, "check_hazard_pads.py"), obj, "--list"],
                         capture_output=True, text=True)
    return out


def test_the_decimate_by_10_bank_kernel_is_built_and_checked(pkg):
    out = _listing(pkg)
    assert out.returncode == 0, out.stderr[-2000:]
    checked = [l.split() for l in out.stdout.splitlines() if l.startswith("checked: bank ")]
    forms = {(int(w[3]), int(w[5]), int(w[7])) for w in checked}
    assert (64, 2, 10) in forms, out.stdout[-2000:]
    assert {f for f in forms if f[2] == 8} == {(32, 2, 8), (32, 4, 8), (64, 2, 8), (64, 4, 8)}
    assert "no packed fp32, every result store padded" in out.stdout


def test_hazard_check_names_the_decimation(pkg, monkeypatch, capsys):
    """a bank symbol without a decimation argument is the decimate-by-8 form; `d 10` from its third argument"""
    sys.path.insert(0, pkg.CSRC)
    try:
        import check_hazard_pads as chk
    finally:
        sys.path.pop(0)
    padded = ["global_store_dwordx2 v[2:3], v[4:5], off nt", "s_nop 1", "s_endpgm"]
    names = ["_ZN4pddc14k_fir_i8x_bankILi64ELi2EEEvNS_10FirI8xBankExi",
             "_ZN4pddc14k_fir_i8x_bankILi64ELi4ELi8EEEvNS_10FirI8xBankExi",
             "_ZN4pddc14k_fir_i8x_bankILi64ELi2ELi10EEEvNS_10FirI8xBankExi"]
    listing = "".join(f"{i * 4096:016x} <{n}>:\n" + "".join("\t" + ins + "\n" for ins in padded) for i, n in enumerate(names))
    monkeypatch.setattr(chk, "disassemble", lambda obj, arch, llvm: listing)
    assert chk.main(["unused.o", "--list"]) == 0
    lines = [l.split() for l in capsys.readouterr().out.splitlines() if l.startswith("checked: bank ")]
    assert [(w[3], w[5], w[6], w[7]) for w in lines] == [("64", "2", "d", "8"), ("64", "4", "d", "8"), ("64", "2", "d", "10")]


def test_header_documents_decimate_by_10_pairs(pkg):
    hdr = open(os.path.join(os.path.dirname(pkg.CSRC), "..", "include", "perseus_ddc.h")).read()
    i = hdr.index("---- bank:")
    para = re.sub(r"\s*\*\s*", " ", hdr[i:hdr.index("#define PDDC_BANK_MAX", i)]).lower()
    assert "decimate-by-10" in para and "pairs" in para and "phase" in para, para
