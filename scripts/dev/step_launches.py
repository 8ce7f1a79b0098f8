"""One steady-state training step of a rocprofv3 --kernel-trace --output-format csv run as `kernel grid block lds` lines.

python scripts/dev/step_launches.py <..._kernel_trace.csv> > launches.txt

The step is what lies between the last two first-layer launches (conv_first_halo_kernel), in host launch order
(Correlation_Id).
"""
import csv
import sys


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    rows.sort(key=lambda r: int(r["Correlation_Id"]))
    first = [i for i, r in enumerate(rows) if "conv_first_halo_kernel" in r["Kernel_Name"]]
    step = rows[first[-2]:first[-1]]
    print("# one steady-state step, ordered by Correlation_Id: kernel grid block lds")
    for r in step:
        print("%s grid=(%s,%s,%s) block=(%s,%s,%s) lds=%s" % (
            r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"],
            r["Workgroup_Size_Y"], r["Workgroup_Size_Z"], r["LDS_Block_Size"]))


main()
