"""The lists of tests/far_cases.py held to what makes them worth running (no GPU): each is a subset of at most 64 cases per place;
at EVERY place it has an accepted case with output (a size query: a positive result); where the entry can refuse it has a refused
case; an encoder's list has in place B an input of 1 KiB or more; and its layout at the GPU's line (tests/device_batch.py:
far_layout with bits = 32, which asserts the allocation invariant) has the straddling chunks, in the input and — where the list has
output — in an output slot with a positive result, at 2^31 and at 2^32."""
import pytest

import device_batch as DB
import far_cases as FC


def test_every_entry_of_the_issue_has_a_list():
    want = {"lz4-decode", "snappy-decode", "lz4-decode-big", "snappy-decode-big", "lz4-sizes", "lz4_dict-decode", "lz4_dict-sizes", "zstd-decode", "zstd-sizes",
            "bgzf-decode", "bgzf-sizes", "bgzf-encode", "blosc-encode", "parquet-pages", "blosc_blosclz-decode", "blosc_zcodecs-decode", "blosc-sizes"}
    want |= {"%s-encode" % c for c in ("lz4", "snappy", "lz4_dict", "deflate_raw", "deflate_zlib", "deflate_gzip", "zstd")}
    want |= {"deflate_%s-%s" % (w, m) for w in ("raw", "zlib", "gzip") for m in ("decode", "sizes")}
    want |= {"orc_%s-%s" % (c, m) for c in ("zlib", "snappy", "lz4", "zstd") for m in ("decode", "sizes", "encode")}
    want |= {"%s_frames-%s" % (f, m) for f in ("lz4", "snappy") for m in ("decode", "sizes", "encode")}
    want |= {"parquet_%s-%s" % (c, m) for c in ("uncompressed", "snappy", "gzip", "zstd", "lz4_raw") for m in ("decode", "decode-crc", "sizes")}
    assert want <= set(FC.LISTS)


@pytest.mark.parametrize("name", sorted(FC.LISTS))
def test_no_list_can_pass_vacuously(name):
    d = FC.far_list(name)
    cs = d["cases"]
    assert 4 <= len(cs) <= 4 * 64
    for p in range(4):
        here = cs[p::4]
        assert len(here) <= 64
        assert any(c.get("verify") or (c["result"] > 0 and (c.get("sized") or c.get("out") or c.get("sha"))) for c in here), (name, "no accepted case with output in place", DB.PLACES[p])
    assert not d["refuses"] or any(c["result"] is not None and c["result"] < 0 for c in cs), (name, "no refused case")
    assert not d["encoder"] or any(len(c["bytes"]) >= 1024 for c in cs[1::4]), (name, "no input of 1 KiB in place B")
    for c in cs:
        assert c.get("sized") or c.get("verify") or c["result"] <= 0 or c.get("out") is not None or c.get("sha"), (name, "an accepted case without expected bytes")
    H, L = 1 << 31, 1 << 32
    for places in DB.FAR_CALLS:
        F = DB.far_layout(name, cs, 32, places)
        for p, line in (("A", H), ("B", L)):
            if p in places:
                s_in, s_out = F.straddlers[p]
                assert len(s_in) == 1 and int(F.in_off[s_in[0]]) < line <= int(F.in_off[s_in[0]]) + int(F.in_len[s_in[0]]) - 1
                assert not d["encoder"] or p == "A" or F.in_len[s_in[0]] >= 1024
                if any(not c.get("sized") for c in cs):
                    assert len(s_out) == 1 and F.want[s_out[0]] > 0 and int(F.out_off[s_out[0]]) < line <= int(F.out_off[s_out[0]]) + int(F.want[s_out[0]]) - 1
        if "C" in places:
            assert int(F.in_off[0]) == L and int(F.out_off[0]) == L
        if "D" in places:
            assert int(F.in_off[2]) == L + (1 << 25) + 5 == int(F.out_off[2])
        assert F.decoys and max(int(o) for o in F.out_off) < L + (1 << 26)


def test_the_big_chunk_lists_straddle_2_pow_32_with_a_slab_mode_output():
    for codec in ("lz4", "snappy"):
        d = FC.far_list("%s-decode-big" % codec)
        F = DB.far_layout(d["name"], d["cases"], 32, DB.FAR_CALLS[0])
        k = F.straddlers["B"][1][0]
        assert F.want[k] > 65536 and int(F.out_off[k]) < 1 << 32 < int(F.out_off[k]) + int(F.want[k])
