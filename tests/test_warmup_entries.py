"""The entries of round 0 composed behind the dry runs, on the emulation library: the same item code as the kernels
(csrc/lz77_warmup.h) in their tile structure (csrc/lz77_warmup_emu.inc) -- the scan of the distance-cache guesses with its carry
across tiles, the walk through runs of segments without commands, the forecast of the static dictionary's death.

Every case runs in one child process under BROTLI_MI355X_SELFTEST=1, where the stage also runs the host's WarmupEnd and forecast
on the same exits and throws if any of the 16 words of an entry or the forecast differs (the closed form of the literal run is
compared with the stepwise loop there as well); the commands must equal the oracle's.  The inputs are those of
test_warmup_entries_gpu.py up to 1 MiB, at the library's own segment size (256 bytes up to 512 KiB, a tile of the scan is 256
segments: 256 KiB of random data is four tiles, 512 KiB eight).  Two exceptions: the emulation's self-test of the candidate rows
fails on a key that owns 65 536 slots or more ("wrap mark mismatch", with or without this code), which the 200 000 zero bytes and
the zero-filled stretch of the 1 MiB mix have.  Those two run without the self-test (commands against the oracle only), and
under it 200 000 bytes of a random 4 KiB piece repeated (copies reach the end of every block there as well, no key longer than
fifty slots) and the first 512 KiB of the mix (runs without commands begin and end inside blocks) stand in for them."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

_CHILD = """
import sys
sys.path.insert(0, %r)
import os, synth
from cmp_lz77 import check
selftest = "BROTLI_MI355X_SELFTEST" in os.environ
text = synth.markov_text((1 << 20) + 4097)
cases = [("markov %%d" %% n, text[:n], 5, None) for n in (256, 512, 768, 65536 + 10)]
if selftest:
    cases.append(("period 4096, 200000", (synth.random_bytes(4096) * 49)[:200000], 5, None))
    cases.append(("mixed 512 KiB", synth.mixed(512 << 10), 5, None))
else:
    cases = [("zeros 200000", bytes(200000), 5, None), ("mixed 1 MiB", synth.mixed(1 << 20), 5, None)]
cases.append(("random 256 KiB", synth.random_bytes(256 << 10), 5, None))
cases.append(("markov hinted", text, 5, len(text)))
cases.append(("markov unhinted", text[:300000], 5, 0))
cases.append(("alice q9", synth.alice(), 9, None))
for name, data, q, hint in cases:
    assert check(name, data, q, 22, size_hint=hint, seg=0), name
print("selftest ok")
"""


def _run(extra_env, selftest=True):
    env = dict(os.environ, **extra_env)
    env.pop("BROTLI_MI355X_SELFTEST", None)
    if selftest:
        env["BROTLI_MI355X_SELFTEST"] = "1"
    r = subprocess.run([sys.executable, "-c", _CHILD % HERE], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "selftest ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_entries_equal_the_hosts_and_commands_the_oracles():
    _run({})


def test_host_switch_keeps_the_host_path_alive():
    _run({"BROTLI_MI355X_HOST_WARMUP": "1"})


def test_inputs_with_a_key_of_65536_slots_without_the_selftest():
    _run({}, selftest=False)
