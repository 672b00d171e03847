"""Diagnostic micro-benchmark of the row gather over row widths and dtypes (not part of the product).
Without arguments it prints, per case: the gather, torch.index_select and a straight copy of the same bytes, as
algorithmic TB/s (4-B index + row read + row write) and as a fraction of the 8 TB/s HBM peak.

    python tools/bench_extract.py --table-dtype f16 --out-dtype f32 [--dim 128] [--rows N] [--table-rows N]
times the converting gather of one pair (ggms_gather_scatter_convert; the same dtype twice is the plain gather), and
    python tools/bench_extract.py --ab [--out FILE]
the comparison behind `feat_out_dtype` in one process, alternating order, table in HBM: (a) plain f16 gather + torch
.float(), (b) fused f16 -> f32, (c) plain f32, (d) f32 -> bf16, and
    python tools/bench_extract.py --fp8-ab [--dim 128 --rows N --table-rows N] [--parent-lib SO] [--alt-lib SO] [--out FILE]
the comparison behind FP8 tables: the six FP8 -> f32 / f16 / bf16 gathers beside the plain f32 gather and the f16 -> X
gathers (of another build of the library too: --parent-lib; --alt-lib adds the FP8 gathers of a trial build), and a
straight copy as the session's copy ceiling, and
    python tools/bench_extract.py --q8row-ab [--dim 128 --rows N --table-rows N] --parent-lib SO [--out FILE]
the comparison behind Q8ROW (row-scaled 8-bit) tables: the three Q8ROW -> f32 / f16 / bf16 gathers beside the f16 -> X
gathers of the parent build's library, the FP8 gathers and a straight copy; condition: a Q8ROW gather is no slower than
the parent's f16 -> X gather of the same output beyond the 3.5 % drift of a session, and
    python tools/bench_extract.py --quantize-ab [--dim 128 --rows N] [--parent-lib SO] [--out FILE]
the comparison behind the row quantiser (ggms_quantize_rows): F32 rows encoded into each of F16, BF16, F8E4M3, F8E5M2
and Q8ROW beside the plain F32 gather of the same rows through an identity index (ggms_gather_scatter; of the parent
build's library with --parent-lib) and a straight device copy of the input bytes; condition: no encode is slower than
that gather beyond the 3.5 % drift of a session."""
import argparse
import ctypes as C
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xgnn_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--table-dtype", choices=["f32", "f16", "bf16", "f8e4m3", "f8e5m2"])
ap.add_argument("--out-dtype", choices=["f32", "f16", "bf16"])
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--rows", type=int, default=2_960_000, help="rows per gather (bench.py's papers100M-shaped batch)")
ap.add_argument("--table-rows", type=int, default=16_000_000)
ap.add_argument("--ab", action="store_true")
ap.add_argument("--fp8-ab", action="store_true")
ap.add_argument("--q8row-ab", action="store_true")
ap.add_argument("--quantize-ab", action="store_true")
ap.add_argument("--parent-lib", help="--fp8-ab / --q8row-ab: a libggms_hip.so of another build, timed beside this one")
ap.add_argument("--alt-lib", help="--fp8-ab: a trial build whose FP8 gathers are timed too")
ap.add_argument("--alt-name", default="trial build")
ap.add_argument("--out", help="--ab / --fp8-ab: also write the report to this file")
args = ap.parse_args()
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f8e4m3": torch.float8_e4m3fn,
      "f8e5m2": torch.float8_e5m2}

dev = torch.device("cuda", 0)
N, n = 2_449_029, 1_280_000


def timeit(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def make_table(table_dtype):
    if table_dtype.startswith("f8"):  # random codes: the decode has no data-dependent branch
        return torch.randint(0, 256, (args.table_rows, args.dim), device=dev, dtype=torch.uint8).view(DT[table_dtype])
    return torch.randn(args.table_rows, args.dim, device=dev).to(DT[table_dtype])


def convert_setup(table_dtype, out_dtype, idx, table=None):
    """(table, out, gather) of one pair; bytes per row = 4 (index) + row read + row written."""
    if table is None:
        table = make_table(table_dtype)
    out = torch.empty((idx.numel(), args.dim), dtype=DT[out_dtype], device=dev)
    return table, out, lambda: ops.gather_scatter_convert(out, table, idx, None)


def run_ab():
    idx = torch.randint(0, args.table_rows, (args.rows,), device=dev, dtype=torch.int32)
    t16, out16, plain16 = convert_setup("f16", "f16", idx)
    _, out32f, fused = convert_setup("f16", "f32", idx, t16)
    t32, out32, plain32 = convert_setup("f32", "f32", idx)
    _, outbf, to_bf16 = convert_setup("f32", "bf16", idx, t32)

    cases = [("a  f16 table, plain gather + torch .float()", lambda: (plain16(), out16.float())),
             ("b  f16 -> f32 fused (8-B load, 16-B store per chunk)", fused),
             ("c  f32 table, plain gather", plain32),
             ("d  f32 -> bf16 fused (16-B load, 8-B store per chunk)", to_bf16)]
    fused()
    plain16()
    assert torch.equal(out32f, out16.float())  # the same rows either way
    times = {name: [] for name, _ in cases}
    for rnd in range(5):  # alternating order: forward, backward, ...
        for name, fn in (cases if rnd % 2 == 0 else cases[::-1]):
            times[name].append(timeit(fn, reps=30))
    med = {k[0]: sorted(v)[len(v) // 2] for k, v in times.items()}
    lines = [f"feat_out_dtype A/B: {args.rows} rows x dim {args.dim}, table {args.table_rows} rows in HBM, one process, "
             f"5 rounds x 30 launches per case in alternating order, median of the rounds (min .. max)",
             f"device: {torch.cuda.get_device_name(0)}"]
    for name, v in times.items():
        lines.append(f"{name:58s} {sorted(v)[len(v) // 2] * 1e3:7.4f} ms  ({min(v) * 1e3:.4f} .. {max(v) * 1e3:.4f})")
    lines += [f"b / a = {med['b'] / med['a']:.3f} (bytes: 0.60)   b / c = {med['b'] / med['c']:.3f} (bytes: 0.75)   "
              f"d / c = {med['d'] / med['c']:.3f} (bytes: 0.75)",
              f"acceptance: b < a: {'PASS' if med['b'] < med['a'] else 'FAIL'};  b <= 1.05 c: "
              f"{'PASS' if med['b'] <= 1.05 * med['c'] else 'FAIL'};  d <= 1.05 c: {'PASS' if med['d'] <= 1.05 * med['c'] else 'FAIL'}"]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def run_fp8_ab():
    """Every case = one ggms_gather_scatter_convert launch on the same index; 5 rounds x 30 launches in alternating
    order; algorithmic bytes = rows x (4 + dim x (table + output element bytes))."""
    idx = torch.randint(0, args.table_rows, (args.rows,), device=dev, dtype=torch.int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def entry(path):
        fn = C.CDLL(path).ggms_gather_scatter_convert
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
        return fn

    from xgnn_amd import _lib
    libs = [("this build", entry(_lib.LIB_PATH))]
    if args.parent_lib:
        libs.append(("parent build", entry(args.parent_lib)))
    tables = {k: make_table(k) for k in ("f32", "f16", "f8e4m3", "f8e5m2")}
    outs = {k: torch.empty((args.rows, args.dim), dtype=DT[k], device=dev) for k in ("f32", "f16", "bf16")}
    cases = []

    def add(name, fn, td, od):
        t, o = tables[td], outs[od]
        code = ops.DTYPE_CODE

        def run():
            rc = fn(o.data_ptr(), t.data_ptr(), idx.data_ptr(), None, args.rows, None, args.dim, code[t.dtype],
                    code[o.dtype], 0xFFFFFFFF, stream)
            assert rc == 0, (name, rc)
        by = args.rows * (4 + args.dim * (t.element_size() + o.element_size()))
        cases.append((name, run, by))

    for lib_name, fn in libs:
        add(f"{lib_name}: f32 plain", fn, "f32", "f32")
        for od in ("f32", "f16", "bf16"):
            add(f"{lib_name}: f16 -> {od}", fn, "f16", od)
    for td in ("f8e4m3", "f8e5m2"):
        for od in ("f32", "f16", "bf16"):
            add(f"this build: {td} -> {od}", libs[0][1], td, od)
    if args.alt_lib:
        fn = entry(args.alt_lib)
        for td in ("f8e4m3", "f8e5m2"):  # the trial differs in the chunk of the f32 output only
            add(f"{args.alt_name}: {td} -> f32", fn, td, "f32")
    # the session's copy ceiling: a straight device copy of the f32 output's size (read + write)
    src_copy = torch.empty_like(outs["f32"])
    cases.append(("straight copy (torch copy_), f32 output size", lambda: outs["f32"].copy_(src_copy),
                  2 * outs["f32"].numel() * 4))
    times = {name: [] for name, _, _ in cases}
    for rnd in range(5):
        for name, fn, _ in (cases if rnd % 2 == 0 else cases[::-1]):
            times[name].append(timeit(fn, reps=30))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    ceiling = cases[-1][2] / med[cases[-1][0]]
    lines = [f"FP8 table A/B: {args.rows} rows x dim {args.dim}, tables of {args.table_rows} rows in HBM, one process, "
             f"5 rounds x 30 launches per case in alternating order, median of the rounds (min .. max; spread = "
             f"(max - min) / median)",
             f"device: {torch.cuda.get_device_name(0)}; copy ceiling of this session: {ceiling / 1e12:.3f} TB/s"]
    for name, _, by in cases:
        v = times[name]
        lines.append(f"{name:46s} {med[name] * 1e3:7.4f} ms  ({min(v) * 1e3:.4f} .. {max(v) * 1e3:.4f}; spread "
                     f"{(max(v) - min(v)) / med[name] * 100:4.1f} %)  {by / med[name] / 1e12:5.2f} TB/s algorithmic = "
                     f"{by / med[name] / ceiling:.3f} of the copy ceiling")
    ref = "parent build" if args.parent_lib else "this build"
    for td in ("f8e4m3", "f8e5m2"):
        for od in ("f32", "f16", "bf16"):
            a, b = med[f"this build: {td} -> {od}"], med[f"{ref}: f16 -> {od}"]
            lines.append(f"{td} -> {od} / {ref}'s f16 -> {od} = {a / b:.3f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def run_q8row_ab():
    """Every case = one ggms_gather_scatter_convert launch on the same index; 5 rounds x 30 launches in alternating
    order; algorithmic bytes = rows x (4 + stored row bytes + dim x output element bytes)."""
    idx = torch.randint(0, args.table_rows, (args.rows,), device=dev, dtype=torch.int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def entry(path):
        fn = C.CDLL(path).ggms_gather_scatter_convert
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
        return fn

    from xgnn_amd import _lib
    this, parent = entry(_lib.LIB_PATH), entry(args.parent_lib) if args.parent_lib else None
    stride = ops.row_bytes(ops.Q8ROW, args.dim)
    q8 = torch.randint(0, 256, (args.table_rows, stride), device=dev, dtype=torch.uint8)
    trailer = torch.empty((args.table_rows, 2), dtype=torch.float32, device=dev)
    trailer[:, 0].uniform_(1e-3, 1e-1)   # scale
    trailer[:, 1].uniform_(-10.0, 10.0)  # bias
    q8[:, stride - 8:] = trailer.view(torch.uint8)
    q8[:, args.dim:stride - 8] = 0
    tables = {"f16": (make_table("f16"), 2, 2 * args.dim), "f8e4m3": (make_table("f8e4m3"), 16, args.dim),
              "f8e5m2": (make_table("f8e5m2"), 17, args.dim), "q8row": (q8, ops.Q8ROW, stride)}
    outs = {k: torch.empty((args.rows, args.dim), dtype=DT[k], device=dev) for k in ("f32", "f16", "bf16")}
    cases = []

    def add(name, fn, td, od):
        (t, code, row), o = tables[td], outs[od]

        def run():
            rc = fn(o.data_ptr(), t.data_ptr(), idx.data_ptr(), None, args.rows, None, args.dim, code,
                    ops.DTYPE_CODE[o.dtype], 0xFFFFFFFF, stream)
            assert rc == 0, (name, rc)
        cases.append((name, run, args.rows * (4 + row + args.dim * o.element_size())))

    for od in ("f32", "f16", "bf16"):  # the three sets alternate: parent's f16 -> X, FP8 -> X, Q8ROW -> X
        if parent:
            add(f"parent build: f16 -> {od}", parent, "f16", od)
        add(f"this build: f16 -> {od}", this, "f16", od)
        for td in ("f8e4m3", "f8e5m2", "q8row"):
            add(f"this build: {td} -> {od}", this, td, od)
    src_copy = torch.empty_like(outs["f32"])
    cases.append(("straight copy (torch copy_), f32 output size", lambda: outs["f32"].copy_(src_copy),
                  2 * outs["f32"].numel() * 4))
    times = {name: [] for name, _, _ in cases}
    for rnd in range(5):
        for name, fn, _ in (cases if rnd % 2 == 0 else cases[::-1]):
            times[name].append(timeit(fn, reps=30))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    ceiling = cases[-1][2] / med[cases[-1][0]]
    lines = [f"Q8ROW table A/B: {args.rows} rows x dim {args.dim} (stored row {stride} B), tables of {args.table_rows} rows "
             f"in HBM, one process, 5 rounds x 30 launches per case in alternating order, median of the rounds (min .. "
             f"max; spread = (max - min) / median)",
             f"device: {torch.cuda.get_device_name(0)}; copy ceiling of this session: {ceiling / 1e12:.3f} TB/s"]
    for name, _, by in cases:
        v = times[name]
        lines.append(f"{name:46s} {med[name] * 1e3:7.4f} ms  ({min(v) * 1e3:.4f} .. {max(v) * 1e3:.4f}; spread "
                     f"{(max(v) - min(v)) / med[name] * 100:4.1f} %)  {by / med[name] / 1e12:5.2f} TB/s algorithmic = "
                     f"{by / med[name] / ceiling:.3f} of the copy ceiling")
    ref = "parent build" if parent else "this build"
    for od in ("f32", "f16", "bf16"):
        a, b = med[f"this build: q8row -> {od}"], med[f"{ref}: f16 -> {od}"]
        lines.append(f"q8row -> {od} / {ref}'s f16 -> {od} = {a / b:.3f}  (bytes: "
                     f"{(4 + stride + args.dim * outs[od].element_size()) / (4 + args.dim * (2 + outs[od].element_size())):.3f}; "
                     f"condition <= 1.035: {'PASS' if a <= 1.035 * b else 'OPEN'})")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def run_quantize_ab():
    """Every case = one launch over the same args.rows x args.dim F32 rows; 5 rounds x 30 launches in alternating order;
    algorithmic bytes = rows x (source row + written row) (+ 4 per row for the gather's index)."""
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    from xgnn_amd import _lib
    src = torch.randn(args.rows, args.dim, device=dev)
    idx = torch.arange(args.rows, device=dev, dtype=torch.int32)
    out32 = torch.empty_like(src)

    def gather(path):
        fn = C.CDLL(path).ggms_gather_scatter
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

        def run():
            rc = fn(out32.data_ptr(), src.data_ptr(), idx.data_ptr(), None, args.rows, None, args.dim, 0, stream)
            assert rc == 0, rc
        return run

    ref = "parent build" if args.parent_lib else "this build"
    row32 = args.dim * 4
    cases = [(f"{ref}: f32 plain gather, identity index", gather(args.parent_lib or _lib.LIB_PATH), args.rows * (4 + 2 * row32))]
    if args.parent_lib:
        cases.append(("this build: f32 plain gather, identity index", gather(_lib.LIB_PATH), args.rows * (4 + 2 * row32)))
    stores = [("f16", torch.float16), ("bf16", torch.bfloat16), ("f8e4m3", torch.float8_e4m3fn),
              ("f8e5m2", torch.float8_e5m2), ("q8row", ops.Q8ROW)]
    for name, dt in stores:
        out = ops.quantize_rows(src, dt)  # (allocated once; Q8ROW's check reads one word back, left out of the timing)
        row = ops.row_bytes(dt, args.dim)
        cases.append((f"this build: f32 -> {name}", lambda dt=dt, out=out: ops.quantize_rows(src, dt, out=out, check=False),
                      args.rows * (row32 + row)))
    cases.append(("straight copy (torch copy_) of the input bytes", lambda: out32.copy_(src), 2 * args.rows * row32))
    times = {name: [] for name, _, _ in cases}
    for rnd in range(5):
        for name, fn, _ in (cases if rnd % 2 == 0 else cases[::-1]):
            times[name].append(timeit(fn, reps=30))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    ceiling = cases[-1][2] / med[cases[-1][0]]
    lines = [f"row quantiser A/B: {args.rows} rows x dim {args.dim}, F32 source in HBM, one process, 5 rounds x 30 launches "
             f"per case in alternating order, median of the rounds (min .. max; spread = (max - min) / median)",
             f"device: {torch.cuda.get_device_name(0)}; copy ceiling of this session: {ceiling / 1e12:.3f} TB/s"]
    for name, _, by in cases:
        v = times[name]
        lines.append(f"{name:50s} {med[name] * 1e3:7.4f} ms  ({min(v) * 1e3:.4f} .. {max(v) * 1e3:.4f}; spread "
                     f"{(max(v) - min(v)) / med[name] * 100:4.1f} %)  {by / med[name] / 1e12:5.2f} TB/s algorithmic = "
                     f"{by / med[name] / ceiling:.3f} of the copy ceiling")
    b = med[cases[0][0]]
    for name, dt in stores:
        a = med[f"this build: f32 -> {name}"]
        lines.append(f"f32 -> {name} / {ref}'s f32 plain gather = {a / b:.3f}  (bytes: "
                     f"{(row32 + ops.row_bytes(dt, args.dim)) / (4 + 2 * row32):.3f}; condition <= 1.035: "
                     f"{'PASS' if a <= 1.035 * b else 'OPEN'})")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if args.quantize_ab:
    run_quantize_ab()
    sys.exit(0)
if args.ab:
    run_ab()
    sys.exit(0)
if args.fp8_ab:
    run_fp8_ab()
    sys.exit(0)
if args.q8row_ab:
    run_q8row_ab()
    sys.exit(0)
if args.table_dtype or args.out_dtype:
    td, od = args.table_dtype or args.out_dtype, args.out_dtype or args.table_dtype
    idx = torch.randint(0, args.table_rows, (args.rows,), device=dev, dtype=torch.int32)
    table, out, fn = convert_setup(td, od, idx)
    t = timeit(fn)
    by = args.rows * (4 + args.dim * (table.element_size() + out.element_size()))
    print(f"{td} -> {od}, {args.rows} rows x dim {args.dim}: {t * 1e6:.1f} us, {by / t / 1e12:.2f} TB/s algorithmic "
          f"({by / t / 8e12:.2f} of 8)")
    sys.exit(0)

idx = torch.randperm(N, device=dev)[:n].to(torch.int32)
idx64 = idx.long()
print("| row | bytes | gather us | gather TB/s (frac of 8) | index_select TB/s | straight copy TB/s |")
print("|---|---|---|---|---|---|")
for name, dtype, dim in [("f32 x 100", torch.float32, 100), ("f32 x 128", torch.float32, 128),
                         ("f32 x 256", torch.float32, 256), ("f32 x 602", torch.float32, 602),
                         ("f16 x 100", torch.float16, 100), ("f16 x 128", torch.float16, 128),
                         ("u8 x 100", torch.uint8, 100), ("i64 x 1", torch.int64, 1), ("f32 x 16", torch.float32, 16)]:
    if dtype.is_floating_point:
        feat = torch.randn(N, dim, device=dev).to(dtype)
    else:
        feat = torch.randint(0, 100, (N, dim), device=dev, dtype=dtype)
    out = torch.empty((n, dim), dtype=dtype, device=dev)
    rb = dim * feat.element_size()
    by = n * (4 + 2 * rb)
    t = timeit(lambda: ops.extract(feat, idx, out=out))
    t_sel = timeit(lambda: torch.index_select(feat, 0, idx64, out=out))
    src = feat[:n]
    t_cp = timeit(lambda: out.copy_(src))
    print(f"| {name} | {rb} | {t * 1e6:.1f} | {by / t / 1e12:.2f} ({by / t / 8e12:.2f}) | {by / t_sel / 1e12:.2f} | "
          f"{2 * n * rb / t_cp / 1e12:.2f} |", flush=True)
    del feat, out
