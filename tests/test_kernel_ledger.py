"""CPU: tools/kernel_ledger.py -- the name normalisation and the fold on a hand-written trace in rocprofv3's column layout
(tests/golden/kernel_trace_sample*.csv: two traced processes), and the guard: every kernel of the built library is in
profiles/kernel_ledger.txt with at least one dispatch, or in EXEMPT with its reason."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sdrangel_amd", "libsdrx.so")
LEDGER = os.path.join(ROOT, "profiles", "kernel_ledger.txt")
SAMPLES = [os.path.join(ROOT, "tests", "golden", f) for f in ("kernel_trace_sample.csv", "kernel_trace_sample_2.csv")]
REGENERATE = ("rocprofv3 --kernel-trace --output-format csv -d DIR -- python -m pytest -m gpu -q && "
              "python tools/kernel_ledger.py fold DIR > profiles/kernel_ledger.txt")

#: kernels that no configuration accepted by a `create` can reach: {name as `symbols` spells it: one-line reason}
EXEMPT = {}

_spec = importlib.util.spec_from_file_location("kernel_ledger", os.path.join(ROOT, "tools", "kernel_ledger.py"))
kl = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kl)


@pytest.mark.parametrize("raw,want", [
    ("void sdrx::decim_fast_kernel<6, 2, 0, false, 4, true>(sdrx::DecimJobs, int, int, int)", "decim_fast_kernel<6,2,0,false,4,true>"),
    ("void sdrx::__device_stub__decim_fast_kernel<6, 2, 0, false, 4, true>(sdrx::DecimJobs, int, int, int)", "decim_fast_kernel<6,2,0,false,4,true>"),
    ("void (anonymous namespace)::wide_pass_kernel<48>((anonymous namespace)::WJob const*)", "wide_pass_kernel<48>"),
    ("(anonymous namespace)::__device_stub__iir_kernel((anonymous namespace)::IirChan*, (anonymous namespace)::IirJob const*)", "iir_kernel"),
    ("sdrx::wfm_prep_kernel(sdrx::WfmChan*, sdrx::WfmBufs const*, int) [clone .kd]", "wfm_prep_kernel"),
    ("sdrx_stream_sum_kernel.kd", "sdrx_stream_sum_kernel"),
    ("__device_stub__sdrx_stream_sum_kernel", "sdrx_stream_sum_kernel"),
    ("void sdrx::be_fft_kernel<1024>(sdrx::BeChan const*, sdrx::BeBufs const*, HIP_vector_type<float, 2u> const*, float const*)", "be_fft_kernel<1024>"),
    ("void sdrx::k<(int)3, 2u, (sdrx::Mode)1>(int)", "k<3,2,1>"),
    ("sdrx_spec::spectrum_avg_kernel(float const*, double*, sdrx_spec::Avg)", "spectrum_avg_kernel"),
])
def test_normalise(raw, want):
    assert kl.normalise(raw) == want


def test_fold_of_the_sample_trace():
    seen = kl.fold(SAMPLES)
    assert seen["decim_fast_kernel<6,2,0,false,4,true>"] == [2, 3, 2]          # 768 / 256 and 256 / 256 in x; 1 and 2 in y
    assert seen["hist_update_kernel"] == [1, 16, 3]
    assert seen["wide_pass_kernel<48>"] == [3, 9, 1]                           # one dispatch in one process, two in the other
    assert seen["wfm_prep_kernel"] == [1, 2, 1]                                # 100 work-items of 64: two workgroups
    assert seen["fdecim_chain_kernel<5,1>"] == [1, 3, 1]
    kernels = ["decim_chain_kernel<6,2,0,0>", "decim_fast_kernel<6,2,0,false,4,true>", "wfm_prep_kernel", "wide_pass_kernel<48>"]
    lines = kl.ledger_lines(kernels, seen)
    assert lines[0] == "# kernels in the library: 4; launched: 3; never: 1"
    assert lines[2:] == ["decim_chain_kernel<6,2,0,0>\tnever", "decim_fast_kernel<6,2,0,false,4,true>\t2\t3x2",
                         "wfm_prep_kernel\t1\t2x1", "wide_pass_kernel<48>\t3\t9x1"]       # other libraries' kernels are left out


def test_ledger_file_round_trip(tmp_path):
    seen = kl.fold(SAMPLES)
    p = tmp_path / "ledger.txt"
    p.write_text("\n".join(kl.ledger_lines(["nobody_kernel", "wide_pass_kernel<48>"], seen)) + "\n")
    assert kl.read_ledger(str(p)) == {"nobody_kernel": (0, 0, 0), "wide_pass_kernel<48>": (3, 9, 1)}
    assert kl.trace_files([os.path.join(ROOT, "tests", "golden")]) == []      # only *kernel_trace.csv counts as a trace


def test_every_kernel_of_the_library_is_launched_by_the_gpu_suite():
    if not os.path.exists(LIB):
        pytest.skip("libsdrx.so is not built")
    kernels = kl.symbols(LIB)
    assert len(kernels) > 300 and "hist_update_kernel" in kernels and all("(" not in k and " " not in k for k in kernels)
    ledger = kl.read_ledger(LEDGER)
    missing = [k for k in kernels if ledger.get(k, (0, 0, 0))[0] < 1 and k not in EXEMPT]
    assert not missing, (f"{len(missing)} kernels of libsdrx.so that no GPU test is known to launch: {missing}.  Add a parity test "
                         f"that reaches them, then regenerate the ledger on a GPU: {REGENERATE}")
    stale = sorted(set(EXEMPT) - set(kernels))
    assert not stale, f"EXEMPT names kernels the library does not have: {stale}"


#: kernels that take a stream or channel index from a block index: the fewest workgroups (x, y) the suite must have given them at once.
#: wide_pass_kernel<64> is left out: it serves sdrx_decim24_* alone, one stream per handle, so its blockIdx.y is always 0
#: (wide_pass_kernel<48>, the same code, runs one row per job of the 24-bit bank).
MIN_GRID = {"decim_fast_kernel<": (3, 2), "decim_chain_kernel<": (3, 2), "hist_update_kernel": (2, 2), "fdecim_chain_kernel<": (2, 1),
            "tree_kernel<": (2, 2), "tree_mx_kernel": (2, 2), "tree_hist_kernel": (2, 2), "wide_pass_kernel<48>": (2, 2),
            "wfm_prep_kernel": (2, 1), "wfm_sched_walk_kernel": (2, 1), "be_sched_dyadic_prep_kernel": (2, 1), "be_schedule_kernel": (2, 1),
            "am_psum_kernel": (2, 1), "nfm_psum_kernel": (2, 1), "ssb_psum_kernel": (2, 1), "udp_psum_kernel": (2, 1),
            # the ChannelAnalyzer bank: four channels per workgroup of the walk, 64 per workgroup of the NCOF phase walk; the channel is
            # blockIdx.y of the group, post, corr and emit kernels and blockIdx.x of the carry
            "chana_walk_kernel": (2, 1), "be_ncof_kernel": (2, 1), "chana_group_kernel": (1, 2), "chana_post_kernel": (1, 2),
            "chana_corr_kernel": (1, 2), "chana_emit_kernel": (1, 2), "chana_carry_kernel": (2, 1)}


def test_block_indexed_kernels_ran_with_more_than_one_workgroup():
    ledger = kl.read_ledger(LEDGER)
    thin = {k: v for k, v in ledger.items() for p, (x, y) in MIN_GRID.items() if k.startswith(p) and v[0] and (v[1] < x or v[2] < y)}
    assert not thin, f"kernels whose largest grid in the GPU suite never left one workgroup where they index by it: {thin}"
    assert all(any(k.startswith(p) for k in ledger) for p in MIN_GRID), "MIN_GRID names a kernel the ledger does not have"
