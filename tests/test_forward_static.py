"""Static properties of the forward launch's generated code (rc_forward.hip), host only.

The embedder half of k_forward keeps its fc1 weight loads in flight from the end of the staging
pass to the first fc1 product.  Two things in the generated code undo that without changing a
result: a flat load (a read through a pointer whose address space the compiler does not know
counts as a memory and an LDS access, so the wait behind it is a full wait on both counters and
drains the weights), and a register count that costs a wave per SIMD.  Both are read here from
the gfx950 assembly, obtained the way scripts/chain_report.py obtains it (hipcc -S with the
build's flags); the test is skipped where the compiler is absent.  For every k_forward
instantiation: no flat loads or stores and no scratch; for the single-window ones the four waves
per SIMD that tests/test_kernel_occupancy.py asks of the built library, and no memory wait
between the fc1 weight request and the first fc1 product."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

MIN_WAVES_SINGLE = 4  # tests/test_kernel_occupancy.py: MIN_WAVES["k_forwardILi1E"]


@pytest.fixture(scope="module")
def forward_kernels(tmp_path_factory):
    import chain_report as cr
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not in the image")
    out = str(tmp_path_factory.mktemp("fwd_asm") / "rc_forward.hip.s")
    cr.assemble(os.path.join(cr.B.CSRC, "rc_forward.hip"), cr.B.CSRC, out)
    ks = cr.parse(out)
    names = cr.demangle(list(ks))
    fwd = dict((names[s], k) for s, k in ks.items() if "k_forward<" in names[s])
    assert len(fwd) == 5, sorted(fwd)  # <1, 512, true>, <1, 512, false>, <1 / 2 / 4, 256, false>
    with open(out) as f:
        LISTING.extend(f.read().splitlines())
    return fwd


LISTING = []  # the assembly file's lines (filled by the fixture)


def _kernel_lines(symbol_part):
    """Labels and instructions of the kernel whose mangled name contains symbol_part."""
    out, on = [], False
    for raw in LISTING:
        line = raw.strip()
        if not on:
            on = raw.startswith("_Z") and symbol_part in raw.split(":")[0]
            continue
        if line.startswith("s_endpgm"):
            break
        if line and line[0] != ";":
            out.append(line)
    assert out, symbol_part
    return out


def _is_load(line):
    return line.startswith("global_load_dword ")


def _waits_for_memory(line):
    return line.startswith("s_waitcnt") and "vmcnt" in line


def test_nothing_waits_for_the_fc1_weights_before_fc1(forward_kernels):
    """From the fc1 weight request (the first run of 48 loads with no memory wait inside it: three
    column steps of 16 rows) to the first fc1 product (the first packed fma that broadcasts one
    operand, the R value; the graph convolution's do not), a memory wait may stand only in a block
    that issues loads of its own (the graph convolution of shapes whose weights are outside LDS) or
    behind the graph convolution's closing barrier, in front of the products.  A wait anywhere else
    drains the request.  This pins what the compiler does today with rc_keep() and rc_wait_loads();
    a compiler that loses it loses time, not results."""
    for symbol in ("k_forwardILi1ELi512ELb1E", "k_forwardILi1ELi512ELb0E", "k_forwardILi1ELi256ELb0E"):
        lines = _kernel_lines(symbol)
        run, start = 0, None
        for i, line in enumerate(lines):
            if _waits_for_memory(line):
                run = 0
            elif _is_load(line):
                run += 1
                if run == 48:
                    start = i + 1
                    break
        assert start is not None, "%s: no 48-load request found" % symbol
        end = next((i for i in range(start, len(lines)) if lines[i].startswith("v_pk_fma_f32") and "op_sel_hi" in lines[i]),
                   None)
        assert end is not None, "%s: no fc1 product found" % symbol
        span = lines[start:end]
        barriers = [i for i, line in enumerate(span) if line.startswith("s_barrier")]
        assert len(barriers) >= 4, (symbol, len(barriers))  # BatchNorm's two, the Chebyshev rows', the graph convolution's
        blocks, cur = [], []
        for i, line in enumerate(span):
            if line.startswith(".LBB") and cur:
                blocks.append(cur)
                cur = []
            cur.append((i, line))
        blocks.append(cur)
        bad = []
        for blk in blocks:
            if any(_is_load(line) for _, line in blk):
                continue
            bad += ["%s: %s" % (symbol, line) for i, line in blk if _waits_for_memory(line) and i < barriers[-1]]
        assert not bad, "\n".join(bad)



def test_forward_has_no_flat_accesses(forward_kernels):
    bad = ["%s: %d flat loads / stores" % (n, k["flat"]) for n, k in forward_kernels.items() if k["flat"]]
    assert not bad, "\n".join(bad)


def test_forward_uses_no_scratch(forward_kernels):
    bad = ["%s: %d bytes of scratch" % (n, k["scratch"]) for n, k in forward_kernels.items() if k["scratch"]]
    assert not bad, "\n".join(bad)


def test_single_window_forward_keeps_four_waves(forward_kernels):
    single = dict((n, k) for n, k in forward_kernels.items() if "k_forward<1," in n)
    assert len(single) == 3, sorted(single)
    bad = []
    for n, k in single.items():
        waves = min(8, 512 // (((k["vgpr"] + 7) // 8) * 8))  # unified register file, granule 8
        if waves < MIN_WAVES_SINGLE or k["occ"] < MIN_WAVES_SINGLE:
            bad.append("%s: %d registers, %d waves per SIMD (compiler: %d)" % (n, k["vgpr"], waves, k["occ"]))
    assert not bad, "\n".join(bad)
