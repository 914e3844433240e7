"""dcvc_build_scale_cdfs / dcvc_build_factorized_cdfs (scale_cdfs_kernel, factorized_cdfs_kernel, quantize_row) on a
real MI355X, called directly as entropy.device_tables calls them, held to the float64 candidate sets of tests/cdf_ref.py:
every row must EQUAL one of the tables that raw counts within E = 0.02 of the float64 p * 65536 give through the exact
integer quantiser -- so a row without an ambiguous bin is right integer for integer, and an off-by-one in the steal
loop, a tail mass over the wrong range, a truncation instead of a rounding or a wrong threshold all fail.  The same
bound holds the reference's own fp32 tables (tests/test_cdf_ref_host.py).  The counts per table are printed and kept in
profiles/device_tables_membership.txt."""
import math

import numpy as np
import pytest
import torch

from tests import cdf_ref as R
from tests.util import oracle_weights
from vcm_ts_amd import entropy as E
from vcm_ts_amd import lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COLS = 104
KIND = {"laplace": 0, "gaussian": 1}


def _fetch(rows, launch):
    # buffers start as garbage-detecting -1: the kernels owe every column of every row, zeros behind the size included
    cdf = torch.full((rows, COLS), -1, dtype=torch.int32, device=DEV)
    sz = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    off = torch.full((rows,), -99, dtype=torch.int32, device=DEV)
    lib.check(launch(cdf.data_ptr(), sz.data_ptr(), off.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream), "launch")
    torch.cuda.synchronize(DEV)
    return cdf.cpu().numpy(), sz.cpu().numpy(), off.cpu().numpy()


def build_scale(scales, kind):
    assert int(lib.hip().dcvc_cdf_table_cols()) == COLS
    s = torch.as_tensor(scales, dtype=torch.float32).to(DEV)
    return _fetch(s.numel(), lambda c, z, o, st: lib.hip().dcvc_build_scale_cdfs(s.data_ptr(), s.numel(), KIND[kind], c, z, o, st))


def build_factorized(block):
    b = torch.as_tensor(block, dtype=torch.float32).contiguous().to(DEV)
    return _fetch(b.shape[1], lambda c, z, o, st: lib.hip().dcvc_build_factorized_cdfs(b.data_ptr(), b.shape[1], c, z, o, st))


def _hold(tag, table, cands, max_undecided=1):
    counts, bad = R.check_table(*table, cands)
    line = (f"{tag:32s}: {counts['identical']:3d} identical {counts['member']:3d} member {counts['undecided']} undecided "
            f"{len(bad)} wrong of {len(cands)} rows")
    print("\n  " + line)
    for r, text in bad[:3]:
        print(f"  {tag} row {r}:\n{text}")
    assert not bad, (tag, [r for r, _ in bad])
    assert counts["undecided"] <= max_undecided and sum(counts.values()) == len(cands), (tag, counts)
    return line


def _levels(kind):
    lmin, _ = E.scale_log_params(kind)
    return torch.exp(torch.linspace(lmin, math.log(E.SCALE_MAX), E.SCALE_LEVELS))


@pytest.mark.parametrize("kind", ["laplace", "gaussian"])
def test_scale_tables_at_the_models_256_levels(kind):
    lv = _levels(kind)
    _hold(f"scale {kind} 256 levels", build_scale(lv, kind), R.scale_candidates(lv.numpy(), kind))


@pytest.mark.parametrize("kind", ["laplace", "gaussian"])
def test_scale_tables_outside_the_models_levels(kind):
    """n_scales != 256; scales below the table (center == 2, narrow bins that round to 0 and go through the steal loop) and
    above it (no i reaches the threshold: 101 symbols and a tail bin with most of the mass); one scale alone."""
    s = R.extra_scales(kind)
    table = build_scale(s, kind)
    _hold(f"scale {kind} {len(s)} scales", table, R.scale_candidates(s, kind), max_undecided=0)
    assert table[1].min() == 7 and table[1].max() == 103
    one = np.array([2.5], np.float32)
    _hold(f"scale {kind} 1 scale", build_scale(one, kind), R.scale_candidates(one, kind), max_undecided=0)


@pytest.mark.parametrize("model,name", [("dmc", "bit_estimator_z"), ("dmc", "bit_estimator_z_mv"), ("intra", "bit_estimator_z")])
def test_factorized_tables_of_the_model_blocks(model, name):
    block = E.factorized_param_block(E.factorized_params(oracle_weights(model), name)).numpy()
    _hold(f"factorized {model} {name}", build_factorized(block), R.factorized_candidates(block))


@pytest.mark.parametrize("name", sorted(R.extra_blocks()))
def test_factorized_tables_of_other_channel_counts(name):
    """C = 1, odd C, C = 256 (the entry's limit: 108 KB of dynamic LDS), and a block with a row shorter than 10 next to
    one at the 101-symbol cap (the padded range of the tail mass differs most from the row's own there)."""
    block = R.extra_blocks()[name]
    table = build_factorized(block)
    _hold(f"factorized {name}", table, R.factorized_candidates(block), max_undecided=0)
    if name == "c8_narrow_and_capped":
        assert table[1].min() - 2 < 10 and table[1].max() - 2 == 101
