"""CPU: the committed wasmsnark_amd/csrc/mad_chain.h -- the form in which the device runs every radix-2^29 product -- is what
tools/gen_mad_chain.py writes, byte for byte: a hand edit, or a generator change without a regenerated header, fails here.  Text only."""
import importlib.util
import os

from conftest import ROOT


def _generator():
    spec = importlib.util.spec_from_file_location("gen_mad_chain", os.path.join(ROOT, "tools", "gen_mad_chain.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)              # (importing renders nothing and writes nothing: the write is behind __main__)
    return mod


def test_committed_header_is_the_generator_output():
    gen = _generator()
    path = os.path.join(ROOT, "wasmsnark_amd", "csrc", "mad_chain.h")
    assert gen.DEFAULT_OUTPUT == path
    with open(path, newline="") as f:
        committed = f.read()
    assert gen.render() == committed


def test_output_option_writes_elsewhere(tmp_path):
    import subprocess
    import sys
    path = os.path.join(ROOT, "wasmsnark_amd", "csrc", "mad_chain.h")
    before = os.stat(path).st_mtime_ns
    out = tmp_path / "chain.h"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_mad_chain.py"), "--output", str(out)])
    assert out.read_text() == _generator().render()
    assert os.stat(path).st_mtime_ns == before
