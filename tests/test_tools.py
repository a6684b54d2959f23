"""The measurement tools that tie the committed profiles to the bench lines
(CPU): prof_summary.py (rocprof kernel trace vs a line's kernel_ms, the sizing
call excluded) and record_pmc.py (an N = 1 line's traffic -> profiles/pmc.json
for N > 1 lines), on synthetic inputs; and isa_diff.py, which vouches for kernels a
refactor must not change, on hand-written assembly."""
import csv
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(kms, kpipe, traffic=3.2e9, n=1):
    return {"metric": "m", "value": 1.0, "n_gpus": n,
            "config": {"workload": "C2-bunny: x", "height": 1080, "spp_per_step": 4, "iters_per_call": 4},
            "roofline": {"kernel": "pt_wf_trace", "kernel_ms": kms, "kernel_ms_pipelined": kpipe, "traffic": traffic,
                         "traffic_source": "live", "l2_hit_rate": 0.8},
            "device": {"library": "pnrt-mi355x 0.2 (gfx950) src abcdef0123456789"}}


def test_prof_summary_excludes_the_sizing_call(tmp_path):
    rows, t = [], 0
    for call in range(3):                    # sizing call (slow), then two timed calls
        # each call starts with its ray generation; the primary pass runs in the
        # first call only (its records are reused while the camera stays)
        prim = [("pt_primary_wf", 0.2)] if call == 0 else []
        for k, ms in prim + [("pt_wf_gen_setup", 1.8)] + [("pt_wf_trace<8, false>", 3.4 if call == 0 else 3.0)] * 4:
            rows.append({"Kernel_Name": f"void {k}(DevScene)", "Start_Timestamp": t, "End_Timestamp": t + int(ms * 1e6)})
            t += int(ms * 1e6) + 1000
    tr = tmp_path / "trace.csv"
    with open(tr, "w", newline="") as f:
        w = csv.DictWriter(f, ["Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        w.writeheader(); w.writerows(rows)
    ln = tmp_path / "line.json"
    line = _line(3.0, 3.1)
    line["config"]["calls"] = "serial"       # a --serial command: compared with the exclusive kernel_ms
    ln.write_text("noise\n" + json.dumps(line) + "\n")
    out = tmp_path / "out.json"
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "prof_summary.py"), str(tr), str(ln), str(out)],
                   check=True, capture_output=True)
    r = json.load(open(out))
    assert r["kernels"]["trace"]["launches"] == 12 and r["kernels"]["trace"]["launches_after_sizing_call"] == 8
    assert abs(r["check"]["rel_diff"]) < 1e-6 and r["check"]["compared_with"] == "kernel_ms"


_ASM = """\t.text
_Z1kv:                                  ; @_Z1kv
; %bb.0:
\ts_load_dword s0, s[0:1], 0x0
{body}
.LBB0_1:                                ; a label, numbered
\ts_cbranch_execz .LBB0_1
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z1kv, .Lfunc_end0-_Z1kv
"""


def test_isa_diff_tells_same_reordered_and_changed():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_diff
    mov, add = "\tv_mov_b32_e32 v1, 0        ; comment", "\tv_add_f32_e32 v2, v0, v0"
    old = isa_diff.kernels(_ASM.format(body=mov + "\n" + add).splitlines())
    assert old["_Z1kv"] == ["s_load_dword s0, s[0:1], 0x0", "v_mov_b32_e32 v1, 0", "v_add_f32_e32 v2, v0, v0", "LBB:",
                            "s_cbranch_execz LBB", "s_endpgm"]
    # the same stream under other label numbers and comments
    same = isa_diff.kernels(_ASM.format(body=mov.split(";")[0] + "\n" + add).replace("LBB0_1", "LBB7_3").splitlines())
    rep, bad = isa_diff.compare(old, same)
    assert bad == 0 and len(rep) == 1 and rep[0].startswith("same ")
    # two instructions swapped: the same multiset, and the diff says which moved
    rep, bad = isa_diff.compare(old, isa_diff.kernels(_ASM.format(body=add + "\n" + mov).splitlines()))
    assert bad == 1 and rep[0].startswith("REORDERED ") and "VALU 2 -> 2" in rep[0]
    assert any(x.strip().startswith("-v_mov_b32") or x.strip().startswith("-v_add_f32") for x in rep[1:])
    # one instruction replaced: not the same work
    rep, bad = isa_diff.compare(old, isa_diff.kernels(_ASM.format(body=mov + "\n\tv_mul_f32_e32 v2, v0, v0").splitlines()))
    assert bad == 1 and rep[0].startswith("DIFFERENT ")
    assert "    -v_add_f32_e32 v2, v0, v0" in rep and "    +v_mul_f32_e32 v2, v0, v0" in rep
    # a long diff is capped, a renamed kernel is found through the name map, a missing one is listed
    many = isa_diff.kernels(_ASM.format(body="\n".join(f"\tv_mov_b32_e32 v{i}, 0" for i in range(200))).splitlines())
    rep, bad = isa_diff.compare(old, {"_Z2k2v": many["_Z1kv"]}, {"_Z1kv": "_Z2k2v"})
    assert bad == 1 and len(rep) == 1 + isa_diff.DIFF_LINES + 1 and "more diff lines" in rep[-1]
    rep, bad = isa_diff.compare(old, {"_Z2k2v": many["_Z1kv"]})
    assert bad == 0 and rep == ["only in old: _Z1kv", "only in new: _Z2k2v"]


def test_record_pmc_keys_by_source_hash(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import record_pmc
    out = tmp_path / "pmc.json"
    monkeypatch.setattr(record_pmc, "OUT", str(out))
    a, b = tmp_path / "a.json", tmp_path / "b.json"
    a.write_text(json.dumps(_line(3.0, 3.5)) + "\n")
    b.write_text(json.dumps(_line(3.0, 3.5, n=2)) + "\n")      # N > 1 lines are not recorded
    record_pmc.main([str(a), str(b)])
    db = json.load(open(out))
    e = db["C2-bunny/trace"]
    assert e["source_hash"] == "abcdef0123456789" and e["frames_per_launch"] == 16 and e["rows"] == 1080
    assert e["bytes_per_launch"] == 3.2e9 and len(db) == 1
