"""sc16 IQ (FOSPHOR_AMD_IQ_SC16), the parts that need no GPU: the header constant and the compiled sc16 kernels' resources."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_kernels.hip")


def test_header_defines_sc16_as_2():
    text = open(os.path.join(ROOT, "include", "fosphor_amd.h")).read()
    m = re.search(r"#define\s+FOSPHOR_AMD_IQ_SC16\s+(\d+)", text)
    assert m and int(m.group(1)) == 2


def test_python_names_the_formats():
    sys.path.insert(0, ROOT)
    from _pkg import gr_fosphor_amd
    from gr_fosphor_amd import core
    assert core.IQ_FORMATS == {"fp32": 0, "fp16": 1, "sc16": 2}
    assert gr_fosphor_amd.Fosphor is core.Fosphor


@pytest.fixture(scope="module")
def kernels_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "kernels.s")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-x", "hip", "--cuda-device-only",
                    "-S", "-o", out, SRC], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


def test_check_k1w_loads_sc16(kernels_asm):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_k1w_loads.py"), "--sc16", kernels_asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 5 and all("k1w_fft_bin" in l and "iq_sc16" in l and l.endswith("ScratchSize 0") for l in lines), r.stdout


def test_sc16_kernels_do_not_spill():
    """-Rpass-analysis=kernel-resource-usage: every sc16 entry point (the format tag iq_sc16 in its name) has 0 bytes of scratch and at most 256 VGPRs."""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-x", "hip", "--cuda-device-only",
                        "-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    cur = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        for key in ("ScratchSize", "VGPRs"):
            m = re.search(r"remark:\s+%s( \[bytes/lane\])?: (\d+)" % key, line)
            if m and cur:
                found.setdefault(cur, {})[key] = int(m.group(2))
    sc16 = {k: v for k, v in found.items() if "iq_sc16" in k}
    assert len(sc16) == 14, sorted(sc16)
    for name, res in sc16.items():
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("VGPRs", 0) <= 256, (name, res)
