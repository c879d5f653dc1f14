"""Helper of tests/test_emu_rowsdev.py, run as a fresh child process: the emulated device row stage on the pipe_two fixture and on the `ordering` design of
tests/rowstage_inputs.py, under whatever environment the parent gave the child BEFORE the emulation library is loaded (a switch the library reads once per process,
such as PHZ_SORT_ONE_LAUNCH, can only be set that way).  Prints one JSON object: {"pipe_two": {file: text}, "ordering": {file: text}}."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, os.path.join(REPO, "oracle"))


def pipe_two():
    from test_emu_rowsdev import _inputs, run_stages
    from test_host_stages import _cases
    from helpers import emu_library
    case, gold, load, cfg = next(c for c in _cases() if c[0] == "pipe_two")
    d, vcf_text, bams = _inputs(case, gold, None)
    out, eng = run_stages(emu_library(), case, load, cfg, vcf_text, bams)
    assert eng.rows_path == "device"
    return out


def ordering():
    import rowstage_inputs as xi
    from helpers import EmuContext, emu_library
    from phaser_amd import vcf
    from test_rowstage_limits import engine_pass, tally_of
    d = xi.ordering()
    ctx = EmuContext(emu_library())
    out, eng = engine_pass(ctx, d, vcf.load_variants(d.vcf_text), tally_of(ctx, d), True, {})
    return out


if __name__ == "__main__":
    print(json.dumps({"pipe_two": pipe_two(), "ordering": ordering()}))
