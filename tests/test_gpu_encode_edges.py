"""The device genotype encoding (pair_table_kernel, key_encode_kernel) and the device BGZF
writer (bgzf_plan_kernel, bgzf_wave_kernel, bgzf_block_kernel) at their limits, on
encode_cases.py's cases (test_encode_cases_cpu.py shows with the oracle alone that each sits
on its edge): 2 | 4 | 5, 16 | 17, 255 | 256 | 257 distinct totals, total ranges 65 535 | 65 536,
8 192 | 8 193 distinct haplotype pairs, packed code tails, bed multiplicity, min_maf, run /
round-robin / shuffled genotype text, and blocks the plan cannot stage.

For every case, and for all of them as regions of one batch, the oracle's rows equal byte
for byte the product's from (a) the dense download, (b) the device reduction, (c) the
reduction + encoding with the codes on the host (encoded_write), (d) the encoding with the
codes left on the device + the device BGZF writer and (e) the same with the codes downloaded
too; keys() equal the oracle's.  Every case also asserts the path it took:
tfbs_batch_encode_stats must give exactly the counters the encoding's limits give the
oracle's keys, and tfbs_ctx_rows_bgzf_blocks the blocks by kernel and the stored ones (the
latter checked against the members' BTYPE bits)."""
import gzip

import pytest

import encode_cases as E
from helpers import T, build_batch
from test_gpu_bgzf import _members

pytestmark = pytest.mark.gpu

CHROM = "chr1"


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def scanner():
    """One Scanner per pattern set, shared by the module's tests."""
    made = {}

    def get(n_ids):
        if n_ids not in made:
            made[n_ids] = T.Scanner(E.pattern_set(n_ids))
        return made[n_ids]

    yield get
    for sc in made.values():
        sc.close()


def _btypes(data):
    """BFINAL | BTYPE << 1 of every member's deflate stream (1: stored, 3: fixed Huffman)."""
    out, i = [], 0
    for bsize, _ in _members(data):
        out.append(data[i + 18] & 7)
        i += bsize
    return out


def _assert_keys(b, okeys):
    assert b.num_regions == len(okeys)
    for i, want in enumerate(okeys):
        got = b.keys(i)
        assert got.keys() == want.keys(), i
        for k in want:
            assert got[k] == want[k], (i, k)


def _bgzf(b, sc, orows, min_maf, device_codes, chunk=None):
    """Rows through the device writer (chunk regions per call); returns the summed block
    counters and the members' BTYPEs."""
    n = b.num_regions
    chunk = chunk or n
    parts, fake, rows = [], 1, 0
    tot = {"blocks": 0, "wave": 0, "stored": 0}
    stats = []
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        b.encode(sc, r0, r1, device_codes=device_codes)
        stats.append(b.encode_stats())
        data, fake, nr, nbytes = b.rows_bgzf(sc, CHROM, min_maf, fake, r0, r1)
        members = _members(data)
        assert sum(m[1] for m in members) == nbytes
        bl = sc.rows_bgzf_blocks()
        assert bl["blocks"] == len(members) and bl["wave"] <= bl["blocks"], bl
        assert bl["stored"] == _btypes(data).count(1), bl
        for k in tot:
            tot[k] += bl[k]
        parts.append(data)
        rows += nr
    data = b"".join(parts)
    assert gzip.decompress(data).decode() == orows
    assert rows == orows.count("\n")
    return tot, _btypes(data), stats


def _assert_blocks(c, tot, btypes):
    if "wave" in c["blocks"]:
        assert tot["wave"] > 0, tot
    if "block" in c["blocks"]:
        assert tot["blocks"] - tot["wave"] > 0, tot
    if "stored" in c["blocks"]:  # really incompressible, not TFBS_BGZF_STORED
        assert tot["stored"] > 0, tot
        assert 1 in btypes and 3 in btypes, btypes
    assert set(btypes) <= {1, 3}


def _run_case(name, scanner, min_maf=0):
    c = E.case(name)
    ps, n, beds, regions = E.materialize(c)
    okeys, orows = E.oracle(name, min_maf)
    want = E.expected_stats(okeys, [E.pair_count(r) for r in c["regions"]])
    assert want["keys"] == len(c["regions"]) * c["n_ids"]
    for path in set(E.region_paths(c)):  # the declared path, from the oracle's keys
        assert want[path] == E.region_paths(c).count(path) * c["n_ids"]
    sc = scanner(c["n_ids"])
    # (a) the dense download
    b = build_batch(ps, n, beds, regions)
    b.scan(sc)
    _assert_keys(b, okeys)
    assert b.rows(CHROM, min_maf)[0] == orows, "dense"
    # (b) the device reduction
    b = build_batch(ps, n, beds, regions)
    b.scan(sc, reduce=True)
    assert b.encode_stats()["keys"] == 0
    _assert_keys(b, okeys)
    assert b.rows(CHROM, min_maf)[0] == orows, "reduce"
    # (c) + the device encoding, codes on the host
    b.encode(sc)
    assert b.encode_stats() == want
    assert b.rows(CHROM, min_maf)[0] == orows, "encode"
    _assert_keys(b, okeys)
    # (d), (e) the device BGZF writer from device codes / with the codes downloaded too
    for device_codes in (True, False):
        tot, btypes, stats = _bgzf(b, sc, orows, min_maf, device_codes)
        assert stats == [want]
        if orows:
            _assert_blocks(c, tot, btypes)
    return b


@pytest.mark.parametrize("name", E.names())
def test_case_vs_oracle(name, scanner):
    _run_case(name, scanner)


@pytest.mark.parametrize("above", [0, 1])
def test_min_maf_on_an_encoded_key(above, scanner):
    """min_maf = the 8-bit key's maf keeps its row (and drops the 4-bit key's), maf + 1 drops it."""
    thr = E.maf_threshold() + above
    _, orows = E.oracle("maf", thr)
    assert orows.count("\n") == 1 - above
    _run_case("maf", scanner, min_maf=thr)


# ---------------------------------------------------------------------------------------
# all cases as regions of one batch

@pytest.fixture(scope="module")
def mixed(scanner):
    """The mixed batch (built once; every test scans and encodes it as it needs), with the
    oracle's keys and rows and each region's number of distinct haplotype pairs."""
    ps, n, beds, regions, where = E.mixed()
    okeys, orows = E.oracle("mixed")
    pair_counts = [E.pair_count(E.case(name)["regions"][j]) for name, j, _ in where]
    sc = scanner(1)
    return build_batch(ps, n, beds, regions), sc, okeys, orows, pair_counts


def test_mixed_batch_dense(scanner):
    ps, n, beds, regions, _ = E.mixed()
    okeys, orows = E.oracle("mixed")
    b = build_batch(ps, n, beds, regions)
    b.scan(scanner(1))
    _assert_keys(b, okeys)
    assert b.rows(CHROM)[0] == orows


def test_mixed_batch_reduce_and_host_codes(mixed):
    b, sc, okeys, orows, pair_counts = mixed
    b.scan(sc, reduce=True)
    _assert_keys(b, okeys)
    assert b.rows(CHROM)[0] == orows, "reduce"
    b.encode(sc)
    want = E.expected_stats(okeys, pair_counts)
    assert want["no_pairs"] == 2 and want["values"] == 4 and want["range"] == 1
    assert want["w2"] and want["w4"] and want["w8"]
    assert b.encode_stats() == want
    assert b.rows(CHROM)[0] == orows, "encode"


@pytest.mark.parametrize("device_codes,chunk", [(True, None), (True, 7), (False, None), (False, 5)])
def test_mixed_batch_bgzf(mixed, device_codes, chunk):
    """One call, and chunks of regions with r0 > 0 (key_encode_kernel's region0); a chunk's
    not-encoded and status != 0 keys sit between encoded ones (code offsets advance by 0)."""
    b, sc, okeys, orows, pair_counts = mixed
    b.scan(sc, reduce=True)
    tot, btypes, stats = _bgzf(b, sc, orows, 0, device_codes, chunk)
    n = b.num_regions
    step = chunk or n
    assert stats == [E.expected_stats(okeys[r0:r0 + step], pair_counts[r0:r0 + step]) for r0 in range(0, n, step)]
    assert tot["wave"] > 0 and tot["stored"] > 0 and 3 in btypes
