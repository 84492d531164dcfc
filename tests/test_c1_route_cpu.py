"""ops.conv1x1_route against the entry points recorded in tests/golden/g19_c1_launches.json (written on an MI355X by
tests/golden/make_c1_launch_golden.py from the revision before the route function existed): for every single-product case
and every form of it, the family the route names is the family of the entry point that ran.  No device: the route reads
switches, the matmul precision and the library's wfae_*_supported predicates, all of them host state."""
import pytest

from tests.c1_golden import GOLDEN, rec


def test_the_golden_holds_every_case_the_recorder_lists():
    assert sorted(GOLDEN["single"]) == sorted(c[0] for c in rec.single_case_ids())
    assert sorted(GOLDEN["block"]) == sorted(c[0] for c in rec.block_case_ids())
    fams = {rec.family_of(n) for g in GOLDEN["single"].values() for n in g["names"]}
    assert fams == {"c1r", "c1rb", "c1b", "c1w", "gemm", None}, fams      # (None: wfae_c1b_weights)


@pytest.mark.parametrize("cfg,switch", sorted({(c[1], c[2] or "") for c in rec.single_case_ids()}))
def test_route_names_the_family_that_ran(cfg, switch):
    from weatherforecastingtoolkit_amd import ops
    checked = 0
    with rec.configured(cfg, switch or None):
        for cid, c, s, m, k, h, w in rec.single_case_ids():
            if (c, s or "") != (cfg, switch):
                continue
            g = GOLDEN["single"][cid]
            assert len(g["forms"]) == len(g["names"])
            for form, entry in zip(g["forms"], g["names"]):
                q = rec.route_query(form, m, k, h * w, rec.CONFIGS[cfg][2])
                if q is None:
                    continue
                assert ops.conv1x1_route(**q) == rec.family_of(entry), (cid, form, entry)
                if form in ("bnred", "bnred_nostore", "bndx"):
                    assert ops.conv1x1_dgrad_bn_route(m, k, h * w) is not None, (cid, form)
                checked += 1
    assert checked >= 27 * 11


def test_dgrad_bn_route_follows_its_switches():
    from weatherforecastingtoolkit_amd import ops
    assert ops.conv1x1_dgrad_bn_route(128, 32, 128) == "bndx" and ops.conv1x1_dgrad_bn_route(32, 128, 128) is None
    assert ops.conv1x1_dgrad_bn_route(128, 32, 128, "bf16") is None and ops.conv1x1_dgrad_bn_route(128, 32, 20) is None
    for switch, want in (("set_c1r_bndx", "bnred"), ("set_c1r_bnred", None), ("set_c1r", None)):
        with rec.configured("highest_split", switch):
            assert ops.conv1x1_dgrad_bn_route(256, 64, 192) == want, switch


def test_peak_table_finds_its_arguments_by_name():
    from weatherforecastingtoolkit_amd import _lib, ops
    decls = _lib.parse_header()
    for entry, fn in ops._PEAK_OF.items():
        args = list(range(1000, 1000 + len(decls[entry][1])))      # distinct values: a wrong position gives another peak class
        assert fn(args) > 0
    names = decls["wfae_conv1x1_fwd_bnact"][2]
    args = [0] * len(names)
    args[names.index("Cout")], args[names.index("Cin")] = 64, 256
    assert ops._PEAK_OF["wfae_conv1x1_fwd_bnact"](args) == ops._gemm_peak(64, 256)
    args[names.index("Cout")], args[names.index("Cin")] = 32, 256      # M < 64: the fp32 instruction
    assert ops._PEAK_OF["wfae_conv1x1_fwd_bnact"](args) == ops.PEAK_FP32_MFMA
