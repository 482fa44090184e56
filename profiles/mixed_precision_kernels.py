"""Per-kernel times of the all-DMA update-block convolutions, fp16 (pf_conv_dma_kernel<NT, KH, KW, WN, true>, mixed_precision)
against bf16x3 (<..., false>), from the rocpd database of one `rocprofv3 --kernel-trace --stats` run of
`profiles/time_mixed_precision.py --trace` (both modes run the same forwards in that process), plus the kernel time per mode of
every other kernel that differs.

    python profiles/mixed_precision_kernels.py <dir>/run_results.db > profiles/r7_mixed_precision_kernels.txt
"""
import re
import sqlite3
import sys
from collections import defaultdict


def main(db):
    c = sqlite3.connect(db)
    st = defaultdict(list)
    for name, dur in c.execute("select name, duration from kernels"):
        st[name].append(dur / 1000.0)
    dma = {}
    for name, ds in st.items():
        m = re.search(r"pf_conv_dma_kernel<(\d+), (\d+), (\d+), (\d+), (true|false)>", name)
        if m:
            dma[(int(m[1]), int(m[2]), int(m[3]), int(m[4]), m[5] == "true")] = ds
    print("all-DMA conv kernel <NT, KH, KW, WN>: launches, mean us, total us  --  bf16x3 | f16 | f16 / bf16x3 (mean)")
    tot = [0.0, 0.0]
    for shape in sorted({k[:4] for k in dma}):
        b, f = dma.get(shape + (False,), []), dma.get(shape + (True,), [])
        mb = sum(b) / len(b) if b else float("nan")
        mf = sum(f) / len(f) if f else float("nan")
        tot[0] += sum(b)
        tot[1] += sum(f)
        print(f"  <{', '.join(map(str, shape))}>  bf16x3 {len(b):5d} {mb:9.1f} {sum(b):11.1f}  |  f16 {len(f):5d} {mf:9.1f} {sum(f):11.1f}"
              f"  |  {mf / mb if b and f else float('nan'):.3f}")
    print(f"  all shapes: bf16x3 {tot[0]:.1f} us, f16 {tot[1]:.1f} us ({tot[1] / tot[0]:.3f})")
    other = [(n, ds) for n, ds in st.items() if "pf_conv_dma_kernel" not in n and ("f16" in n or "split" in n)]
    for n, ds in sorted(other):
        print(f"  {n[:90]}: {len(ds)} launches, mean {sum(ds) / len(ds):.1f} us")


if __name__ == "__main__":
    main(sys.argv[1])
