"""Progressive render sessions without a GPU: the header declares the entries and the Python mirror binds them, the checkpoint header parses to the
documented fields, and the command line's rules between the flags hold."""
import ctypes as C
import os
import re
import struct

import pytest

import gi_raytracer_amd as gi
import gi_raytracer_amd.__main__ as cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gi_progressive_begin", "gi_progressive_step_device", "gi_progressive_step_host", "gi_progressive_status", "gi_progressive_state_bytes",
           "gi_progressive_save", "gi_progressive_restore", "gi_progressive_end")


def test_header_declares_and_the_library_exports_the_eight_entries():
    txt = open(os.path.join(ROOT, "include/gi_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\bint\s+(gi_progressive_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(ENTRIES)
    L = gi.lib()
    for n in ENTRIES:
        assert n in gi.ABI_SYMBOLS and hasattr(L, n), n
        assert getattr(L, n).argtypes[0] is C.c_void_p, n          # bound with argument types: the context first
    assert len(L.gi_progressive_step_host.argtypes) == 6 and L.gi_progressive_step_host.argtypes[1] is C.c_int32
    assert L.gi_progressive_save.argtypes[2] is C.c_int64 and L.gi_progressive_restore.argtypes[2] is C.c_int64


def test_python_surface():
    for name in ("step", "frame", "save", "close", "sample_end", "pixels_wanting", "done", "__enter__", "__exit__"):
        assert hasattr(gi.ProgressiveRender, name), name
    assert callable(gi.RayTracer.progressive) and callable(gi.RayTracer.resume)


def hand_made_blob(n_records=3, **over):
    """A checkpoint written from the layout include/gi_hip.h documents, field by field."""
    f = dict(magic=b"GIPROGR\0", version=1, header_bytes=192, cam=[10.0, 5.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0], sensor_diag=0.035, focal_dist=0.04,
             width=3, height=1, stripe_h=1, stripe_rank=0, stripe_world=1, min_samples=7, max_samples=7, noise_thresh=0.0015, seed=0x9E3779B97F4A7C15,
             schedule=0, sample_end=3, n_records=n_records, record_bytes=72, n_entity=12, n_node=9, n_photon=345)
    f.update(over)
    b = f["magic"] + struct.pack("<II", f["version"], f["header_bytes"])
    b += struct.pack("<11d", *f["cam"], f["sensor_diag"], f["focal_dist"])
    b += struct.pack("<7i", f["width"], f["height"], f["stripe_h"], f["stripe_rank"], f["stripe_world"], f["min_samples"], f["max_samples"]) + b"\0" * 4
    b += struct.pack("<dQ", f["noise_thresh"], f["seed"])
    b += struct.pack("<iiQII", f["schedule"], f["sample_end"], f["n_records"], f["record_bytes"], 0)
    b += struct.pack("<iiii", f["n_entity"], f["n_node"], f["n_photon"], 0)
    assert len(b) == 192
    rec = struct.pack("<7d4i", 0.25, 0.5, 0.75, 0.2, 0.4, 0.6, 0.01, 3, 3, 0, 0)
    assert len(rec) == 72
    return b + rec * n_records, f


def test_checkpoint_header_parses_to_the_documented_fields():
    assert struct.calcsize(gi.CHECKPOINT_HEADER) == 192 and gi.CHECKPOINT_RECORD_BYTES == 72
    assert C.sizeof(gi.RenderParams) == 136                    # the header carries the structure as it lies in memory: offsets 16 .. 152
    blob, f = hand_made_blob()
    h = gi.parse_checkpoint_header(blob)
    for k in ("version", "header_bytes", "sensor_diag", "focal_dist", "width", "height", "stripe_h", "stripe_rank", "stripe_world", "min_samples", "max_samples",
              "noise_thresh", "seed", "schedule", "sample_end", "n_records", "record_bytes", "n_entity", "n_node", "n_photon"):
        assert h[k] == f[k], k
    assert list(h["cam_pos"] + h["cam_up"] + h["cam_forward"]) == f["cam"]
    # the same bytes read as the C structure
    p = gi.RenderParams.from_buffer_copy(blob[16:152])
    assert (p.width, p.height, p.min_samples, p.max_samples, p.noise_thresh, p.seed) == (3, 1, 7, 7, 0.0015, 0x9E3779B97F4A7C15) and list(p.cam_pos) == [10.0, 5.0, 0.0]


@pytest.mark.parametrize("change", [lambda b: b[:-1], lambda b: b"X" + b[1:], lambda b: b[:8] + struct.pack("<I", 2) + b[12:], lambda b: b[:100],
                                    lambda b: b[:168] + struct.pack("<I", 80) + b[172:], lambda b: b + b"\0"],
                         ids=["cut", "magic", "version", "short", "record-size", "long"])
def test_damaged_checkpoints_are_refused(change):
    blob, _ = hand_made_blob()
    with pytest.raises(ValueError):
        gi.parse_checkpoint_header(change(blob))


@pytest.mark.parametrize("flags, message", [(["--checkpoint", "c.bin"], "need --progressive"), (["--time-limit", "5"], "need --progressive"),
                                            (["--progressive", "0"], "at least 1"), (["--progressive", "-3"], "at least 1"),
                                            (["--progressive", "2", "--time-limit", "-1"], ">= 0"), (["--progressive", "two"], "invalid int value"),
                                            (["--progressive", "2", "--time-limit", "nan"], ">= 0")],
                         ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_cli_refuses_flag_combinations_before_touching_a_device(flags, message, capsys):
    """Each case names the rule it breaks: the exit status is argparse's 2 and the error text is that rule's (an unknown flag has the status too)."""
    with pytest.raises(SystemExit) as e:
        cli.main(["no_such_scene.scn"] + flags)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_cli_accepts_the_progressive_flags():
    ap = cli.parser()
    a = ap.parse_args(["s.scn", "--progressive", "8", "--time-limit", "0", "--checkpoint", "c.bin"])
    cli.check_args(ap, a)
    assert (a.progressive, a.time_limit, a.checkpoint) == (8, 0.0, "c.bin")
    a = ap.parse_args(["s.scn"])
    cli.check_args(ap, a)
    assert a.progressive is None and a.time_limit is None and a.checkpoint is None


def test_replace_file_leaves_no_partial_file(tmp_path):
    path = tmp_path / "f.bin"
    path.write_bytes(b"old")

    def failing(t):
        open(t, "wb").write(b"ne")
        raise RuntimeError("interrupted")

    with pytest.raises(RuntimeError):
        cli.replace_file(str(path), failing)
    assert path.read_bytes() == b"old" and sorted(os.listdir(tmp_path)) == ["f.bin"]      # the file a viewer reads is whole, the partial one is gone
    cli.replace_file(str(path), lambda t: open(t, "wb").write(b"new"))
    assert path.read_bytes() == b"new" and sorted(os.listdir(tmp_path)) == ["f.bin"]
