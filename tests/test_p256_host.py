"""The device verify path's arithmetic (babble_amd/csrc/hge_p256.h, shared by host and
device) against OpenSSL on the CPU (tests/abi/hge_p256_test.cpp): Montgomery arithmetic
modulo the field prime and the group order on edge operands and random ones, Jacobian
double / add / mixed add with P + P, P + (-P) and infinity on either side, the windowed
double-scalar multiplication against EC_POINT_mul, key decoding against
EC_POINT_oct2point, p256_ecdsa_verify_digest against ECDSA_do_verify (valid signatures,
r or s of 0 or n, flipped bits, another key, digest 0, Q = G and Q = -G with e = r), and
SHA-256 at every length from 0 to 130.  Plain host C++ and libcrypto, no engine and no
device: this runs in the CPU suite."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_p256_header_against_openssl():
    exe = os.path.join(ROOT, "build", "hge_p256_test")
    assert os.path.exists(exe), "built by __graft_entry__.build() (babble_amd/csrc/Makefile)"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.startswith("ok "), out.stdout
    # 33 edge operands squared x 4 checks x 2 moduli alone
    assert int(out.stdout.split()[1]) > 2 * 33 * 33 * 4
