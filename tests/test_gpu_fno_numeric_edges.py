"""The cases of tests/test_fno_numeric_edges.py through the device (csrc/hc_fno_kernels.hip, hc_api_fno.cpp), on both of its routes:
the lines' 256-bit text-order keys at every digit count and sign of every column and on both sides of the three splits between key
words (kid2 at bit 6, kp2 at bit 22, kl1 at bit 13), the type and orientation bits, the pair sort of the walk over 2 * id_bits
bits up to all 62 and at the 8-bit passes' boundaries, the nodes_to_SR sort at a power of two of vertices, and the thresholds past
which the host form takes the call.  Every case asserts the bytes against R1 / R2, the counters against the host form's and the
level the route must report."""
import os

import pytest

from haploconduct_amd import fno as F
from tests import _fno as T
from tests import test_fno_numeric_edges as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def olib():
    return T.load_oracle()


@pytest.fixture(params=["walk on the device", "walk on the host threads"])
def on_device(request):
    """Both device routes of FNO=1, as in tests/test_gpu_fno.py: level 2, or level 1 under HC_FNO_WALK=host."""
    os.environ["HC_FNO"] = "device"
    if request.param.endswith("host threads"):
        os.environ["HC_FNO_WALK"] = "host"
    yield 1 if request.param.endswith("host threads") else 2
    os.environ.pop("HC_FNO", None)
    os.environ.pop("HC_FNO_WALK", None)


@pytest.mark.parametrize("pair", list(cases.PAIRS))
@pytest.mark.parametrize("field", T.LADDER_FIELDS)
def test_one_field_ladders(on_device, field, pair):
    cases.case_ladder(field, pair, on_device)


@pytest.mark.parametrize("field", list(T.SPLIT_BIT))
def test_straddles(on_device, field):
    cases.case_straddle(field, on_device)


def test_tail_bits_and_repeats(on_device):
    cases.case_tail(on_device)


def test_product_scenario(on_device):
    cases.case_product(on_device)


def test_product_scenario_with_ten_digit_ids_through_the_device_walk(on_device):
    """No super-read, so overlaps_found is never indexed and new_read_count only sets the width of the pair sort: at 2^31 the walk
    stays on the device and copies ids of ten digits itself."""
    cases.case_product(on_device, new_read_count=2 ** 31)


@pytest.mark.parametrize("flags", cases.FLAG_SETS)
@pytest.mark.parametrize("seed", range(8))
def test_sparse_ids_through_the_walk(olib, on_device, seed, flags):
    cases.case_sparse_ids(olib, seed, flags, on_device)


@pytest.mark.parametrize("new_read_count", cases.PASS_BOUNDARIES)
def test_pair_sort_width(olib, on_device, new_read_count):
    cases.case_pair_sort_width(olib, new_read_count, on_device)


@pytest.mark.parametrize("n_nodes", cases.NODE_COUNTS)
def test_vertex_count_at_a_power_of_two(olib, on_device, n_nodes):
    cases.case_node_bits(olib, n_nodes, on_device)


def test_largest_id_of_the_keys_and_the_first_beyond(on_device):
    cases.case_threshold_id(on_device)


def test_largest_percentage_of_the_keys_and_the_first_beyond(on_device):
    cases.case_threshold_perc(on_device)


@pytest.mark.parametrize("flags", [0, F.NO_INCLUSIONS])
@pytest.mark.parametrize("seed", range(8))
def test_fno3_sparse_ids(olib, on_device, seed, flags):
    cases.case_fno3(olib, seed, flags, on_device)
