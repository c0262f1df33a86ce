"""CPU-only: the oracle search of test_tail_block_clean.py (tests/_tail_block_clean.py).  Every event the GPU test names must
be found in the family it is named for within the seeds the GPU test uses, so that a change to a generator cannot silently
empty the GPU test; the located rounds must be what they are named for; and the count of clean block rounds
(tools/tail_block_clean.py, profiles/tail_block_clean.txt) is pinned on a small config."""
import os
import re
import subprocess

import numpy as np
import pytest

import _tail_block_clean as tc
from sslap_amd import synth


@pytest.mark.parametrize("family", list(tc.REQUIRED), ids=lambda f: "%d-%s-%s" % f[:3])
def test_every_event_is_found(family):
    found, missing = tc.locate(family, tc.REQUIRED[family])
    assert not missing, missing
    assert all(sd in tc.SEEDS and r >= 1 for sd, r in found.values())


def test_without_lines_and_batch_events():
    found, missing = tc.locate(tc.LANES, tc.NO_LINES)
    assert not missing, missing
    for key, cap in zip(tc.BATCH_KEYS, tc.BATCH_CAPS):
        assert cap is None or tc.trace(key)[2].get(cap), (key, cap)
    assert len(set(k[0] for k in tc.BATCH_KEYS)) == 1


def test_located_rounds_are_what_they_say():
    n, kind, prob, opts = tc.LANES
    found, _ = tc.locate(tc.LANES, tc.REQUIRED[tc.LANES])
    for name, (seed, r) in found.items():
        ev = tc.trace((n, seed, kind, prob, opts))[2]
        assert r in ev["block"], name
        if name.startswith("clean K") or name in ("clean odd K", "dirty then clean"):
            assert r in ev["clean"], name
        if name in ("clean then dirty", "K falls by one", "hole in the last slot"):
            assert r not in ev["clean"], name
    ev = tc.trace((n, 1, kind, prob, opts))[2]
    assert len(ev["clean"]) >= 100  # the lanes family: clean rounds at every K, between the rounds that end a lane's war


def test_colliding_columns_share_the_hash():
    n, kind, prob, opts = tc.LANES_COLLIDE
    loc = tc.trace((n, 1, kind, prob, opts))[0]
    cols = np.unique(loc[:, 1])
    assert len(cols) == n and len(set(tc.clean_hash(j) for j in cols)) == n // 2


def test_rows_without_a_line():
    n, kind, prob, opts = tc.LANES_LONG
    loc = tc.trace((n, 1, kind, prob, opts))[0]
    lens = np.bincount(loc[:, 0])
    assert (lens > tc.ROW_NEVER_CACHED).sum() == 25 and (lens[lens <= tc.ROW_NEVER_CACHED] == 3).all()


def test_count_of_clean_block_rounds():
    """The step-0 count of the pull request that added the clean path, on the smallest BASELINE config (its block rounds
    are those of a 5 000 x 5 000 problem: far fewer clean ones than at C2 / C3, see profiles/tail_block_clean.txt)."""
    loc, val = synth.gen_config("C1")
    c = tc.count_clean(loc, val, "max")
    assert c["rounds"] == 7553
    assert c["K<=64"] == [419, 224, 39, 156] and c["K>64"] == [110, 2, 58, 50]
    for row in (c["K<=64"], c["K>64"]):
        assert row[0] == sum(row[1:])


@pytest.mark.parametrize("family", [tc.LANES_WIDE, tc.LANES_WIDE_MIN, tc.LANES_WIDE_64], ids=["max", "min", "slot64"])
def test_rows_whose_lines_get_spent(family):
    """The located rounds are clean block rounds with a bidder whose row is longer than a line and short enough to keep one
    (30 < 42 <= 256): a miss of such a row rebuilds its line."""
    n, kind, prob, opts = family
    loc, val, ev, total = tc.trace((n, 1, kind, prob, opts))
    lens = np.bincount(loc[:, 0])
    assert (lens == tc.WIDE).sum() == tc.WIDE and ((lens == tc.WIDE) | (lens == 3)).all()
    assert tc.LINE < tc.WIDE <= tc.ROW_NEVER_CACHED
    located = [r for r in ev[tc.REBUILD] if r - 1 in ev["block"]]
    assert len(located) >= 100 and set(located) <= set(ev["clean"])
    wide = loc[lens[loc[:, 0]] == tc.WIDE]
    v = val[lens[loc[:, 0]] == tc.WIDE]
    v = v if prob == "max" else -v
    assert len(np.unique(wide[:, 1])) == tc.WIDE  # one lane: its persons value its objects alone
    assert np.ptp(np.sort(v.reshape(tc.WIDE, tc.WIDE), axis=1)[:, 1:]) < 2.0 ** -9  # 41 near-equal edges per row, far below eps


def test_tail_kernels_fit_their_registers(built_lib, tmp_path):
    """Read off the built library's gfx950 code object: no tail kernel uses scratch, and no 1024-thread instance needs more
    than the 128 VGPRs such a workgroup leaves a wavefront.  (The block instances stay there only because the slot-indexed
    LDS addresses are formed inside their blocks -- slot_index_here, kernels_tail.hpp -- and the clean table shares hKey.)"""
    from sslap_amd import _lib, build
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "lib", "llvm", "bin")
    fat, elf = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.elf")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, _lib.LIB_PATH, os.devnull])
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf])
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], capture_output=True, text=True, check=True).stdout
    roles = ("12k_tail_blockI", "11k_tail_teamI", "11k_tail_pairI", "14k_tail_nolinesI")
    kernels = [k for k in re.split(r"\n  - \.agpr_count:", notes) if re.search(r"\.name:\s+\S*\d+k_tail_\w+I", k)]
    assert len(kernels) >= 24  # 2 layouts x 4 kernels x (entry, k_batched, k_batched_ptr)
    field = lambda k, name: int(re.search(r"\.%s:\s+(\d+)" % name, k).group(1))
    names = [re.search(r"\.name:\s+(\S+)", k).group(1) for k in kernels]
    for role in roles:  # each kernel for both layouts, by itself and in both batched wrappers
        for layout in ("8EdgesF32E", "8EdgesF64E"):
            for wrapper in ("_ZN7misslap%s", "_ZN7misslap9k_batchedINS_%s", "_ZN7misslap13k_batched_ptrINS_%s"):
                assert any(n.startswith(wrapper % role + "NS_" + layout) for n in names), (role, layout, wrapper)
    for k, name in zip(kernels, names):
        assert field(k, "private_segment_fixed_size") == 0 and field(k, "vgpr_spill_count") == 0, name
        if field(k, "max_flat_workgroup_size") == 1024:
            assert field(k, "vgpr_count") <= 128, name
