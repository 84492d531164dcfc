"""Launch traces of the 1x1 products against tests/golden/g19_c1_launches.json: the cases of
tests/golden/make_c1_launch_golden.py replayed on this tree.  Per case (i) the entry points called, in order, and the
SHA-256 of their canonical argument lines equal the recorded ones; (ii) for single products, the family
ops.conv1x1_route names is the family of the entry point recorded.  A route that quietly falls back to another kernel
family fails here by name, whatever its results look like."""
import pytest

from tests.c1_golden import GOLDEN, rec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg,switch", sorted({(c[1], c[2] or "") for c in rec.single_case_ids()}))
def test_single_products_launch_what_was_recorded(dev, cfg, switch):
    from weatherforecastingtoolkit_amd import ops
    for cid, c, s, m, k, h, w in rec.single_case_ids():
        if (c, s or "") != (cfg, switch):
            continue
        forms, lines = rec.run_single(dev, c, s, m, k, h, w)
        got, want = rec.digest(lines), GOLDEN["single"][cid]
        assert forms == want["forms"] and got["names"] == want["names"], (cid, forms, got["names"], want["names"])
        assert got["sha256"] == want["sha256"], (cid, lines)
        with rec.configured(c, s):
            for form, entry in zip(forms, got["names"]):
                q = rec.route_query(form, m, k, h * w, rec.CONFIGS[c][2])
                assert q is None or ops.conv1x1_route(**q) == rec.family_of(entry), (cid, form, entry)


@pytest.mark.parametrize("cfg", sorted(rec.CONFIGS))
def test_bottleneck_blocks_launch_what_was_recorded(dev, cfg):
    for cid, c, *args in rec.block_case_ids():
        if c != cfg:
            continue
        lines = rec.run_block(dev, c, *args)
        got, want = rec.digest(lines), GOLDEN["block"][cid]
        assert got["names"] == want["names"], (cid, got["names"], want["names"])
        assert got["sha256"] == want["sha256"], (cid, lines)
