"""k_bp's shared-reciprocal division (csrc/div_shared.h) on the CPU: tools/div_model.cc runs the very
header with a modelled hardware seed, (1 / Q)(1 + d) with d uniform in +-eps0, over numerators and
denominators from the kernel's own polynomials (fast_tanh over |y| <= 9.94, fast_atanh over
|x| <= 1.0073, a share scaled down to 2^-100 / 2^-600, a share of denominators with an all-ones or a
1.0...01 significand).  Condition: not one quotient differs in bits from the host's x / y.

eps0 = 2^-23 is v_rcp_f64's documented accuracy; 2^-20 shows the margin."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tools", "div_model.cc")
CXXFLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"]
N_DIV = 20_000_000


def _cxx():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a host C++ compiler (g++) is required"
    return cxx


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("div_model") / "div_model")
    subprocess.run([_cxx(), "-O2", *CXXFLAGS, SRC, "-o", exe], check=True)
    return exe


def _mismatches(exe, k, log2_eps, n):
    r = subprocess.run([exe, str(k), str(log2_eps), str(n), str(1000 + 10 * k - log2_eps)],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode in (0, 1), (r.returncode, r.stderr)
    last = r.stdout.strip().splitlines()[-1]
    fields = dict(f.split("=", 1) for f in last.split())
    assert int(fields["divisions"]) >= n
    return int(fields["mismatches"])


@pytest.mark.parametrize("log2_eps", [-23, -20])
@pytest.mark.parametrize("k", [3, 9])
def test_every_quotient_is_correctly_rounded(model, k, log2_eps):
    assert _mismatches(model, k, log2_eps, N_DIV) == 0


def test_model_detects_a_bad_seed(model):
    """The comparison is live: a seed good to only 2^-4 leaves the reciprocals short of an ulp."""
    assert _mismatches(model, 9, -4, 200_000) > 0


def test_under_address_and_undefined_sanitizers(tmp_path):
    """The same stand-alone program under ASan + UBSan (host code, no GPU): the header indexes its
    register arrays with compile-time bounds only, and this run proves it."""
    exe = str(tmp_path / "div_model_san")
    r = subprocess.run([_cxx(), "-O1", "-g", *CXXFLAGS, "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the host compiler cannot link the sanitizer runtimes: " + r.stderr[-300:])
    for k in (3, 9):
        assert _mismatches(exe, k, -23, 300_000) == 0
