"""Child process of tests/test_gpu_key_file.py: loads ONE shard of a key file and reports how far the process's resident set rose
while it did (VmHWM after - VmRSS before), in bytes.  A fresh process: the peak is this load's, not the key generator's.  Also lists the anonymous
mappings the load created (/proc/self/smaps before and after): the test tells fixed-size host blocks from memory that grows with the key."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def status(field):
    for line in open("/proc/self/status"):
        if line.startswith(field + ":"):
            return int(line.split()[1]) * 1024
    return 0


def anon_mappings():
    out, cur = {}, None
    for line in open("/proc/self/smaps"):
        parts = line.split()
        if parts and "-" in parts[0] and not parts[0].endswith(":"):
            lo, hi = (int(x, 16) for x in parts[0].split("-"))
            cur = (parts[0], hi - lo) if len(parts) == 5 else None          # (no path name: anonymous)
            if cur:
                out[cur] = 0
        elif cur and parts[0] == "Rss:":
            out[cur] = int(parts[1]) * 1024
    return out


path, rank, world, hlog = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
import torch  # noqa: E402,F401
import wasmsnark_amd  # noqa: E402

bn = wasmsnark_amd.build(device=0)
warm = bn.load_key(path=sys.argv[5]) if len(sys.argv) > 5 else None      # (a small key first: staging ring, code objects, allocator pools)
if warm is not None:
    warm.free()
maps_before = anon_mappings()
before = status("VmRSS")
key = bn.load_key(path=path, shard=(rank, world), h_interleave_log=hlog, wait_tables=False)
peak = status("VmHWM")
new = [{"bytes": k[1], "rss": v} for k, v in anon_mappings().items() if k not in maps_before and v]
print(json.dumps({"rss_before": before, "hwm_after": peak, "rise": max(0, peak - before), "file_bytes": os.path.getsize(path),
                  "shard": key.shard, "load_ms": key.load_ms, "new_anon_mappings": new}))
