"""The device haplotype grouper (build_gpu.hip: mask_scatter_kernel, mask_group_kernel,
GpuGrouper::group) at its limits: the calls of tests/group_cases.py on the HIP grouper
equal the reference of its own operation (tests/group_ref.py) exactly -- which masks,
in which order, with which counts and which membership row, per region of a launch --
and the batches of tests/test_group_cases_cpu.py built on device 0 are the plain host
batch and scan to its keys and rows.  What each case reaches is proven in the CPU file."""
import pytest

from helpers import T
from test_group_cases_cpu import (CASE_NAMES, check_calls, edge_batches, limit_batches, reference,  # noqa: F401
                                  refusals, synth_batches)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")


@pytest.fixture(scope="module")
def grouper():
    g = T.Grouper(0)
    yield g
    g.close()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_grouper_is_the_reference(name, reference):  # noqa: F811
    g = T.Grouper(0)  # a fresh handle: scratch and rows sized by this case alone
    try:
        check_calls(g, name, reference)
    finally:
        g.close()


def test_every_case_on_one_handle(grouper, reference):  # noqa: F811
    """Scratch growth, the zeroed masks and the recycled rows across every case's calls,
    forwards and backwards."""
    for name in CASE_NAMES + CASE_NAMES[::-1]:
        check_calls(grouper, name, reference)


def test_refused_input_is_not_launched(grouper):
    refusals(grouper)


def same_scan(ps, host, dev):
    """Keys and rows after scan(reduce, encode): the device batch's membership read in
    place by the pair tables and fetched by rows()."""
    sc = T.Scanner(ps)
    try:
        host.scan(sc, reduce=True, encode=True)
        want, _ = host.rows("chr1")
        want_keys = [host.keys(i) for i in range(host.num_regions)]
        dev.scan(sc, reduce=True, encode=True)
        got, _ = dev.rows("chr1")
        got_keys = [dev.keys(i) for i in range(dev.num_regions)]
    finally:
        sc.close()
    assert got_keys == want_keys
    assert got == want


def test_edge_regions_held_padded_rows(tmp_path):
    """The 13 crafted regions in one release, n_samples = 1501: eleven regions in one
    launch (one overflowing), rows of 3002 entries padded to 3008."""
    ps, host, dev = edge_batches(tmp_path, 1501, 0)
    same_scan(ps, host, dev)


def test_limit_regions_in_one_chunk(tmp_path):
    ps, host, dev = limit_batches(tmp_path, 0)
    same_scan(ps, host, dev)


@pytest.mark.parametrize("cap", ["1", "7"])
@pytest.mark.parametrize("indel", [0, 3])
def test_chunk_loop_takes_further_turns(tmp_path, monkeypatch, indel, cap):
    monkeypatch.setenv("TFBS_GROUP_REGIONS", cap)
    ps, host, dev = synth_batches(tmp_path, 101, indel, 130, 0, calls=-(-130 // int(cap)))
    same_scan(ps, host, dev)
