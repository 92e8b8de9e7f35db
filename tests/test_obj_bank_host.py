"""CPU: the host side of cached obj_tx rows and the object-transformer bank - vog_batch with its new field and the new
vog_objrestore_args against gcc's layout, the new exports, the argument errors that are raised before anything touches a device,
the engine's key validation, the footprint arithmetic and the command line."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module("vognet-pytorch_amd.lib")
dls = importlib.import_module("vognet-pytorch_amd.dat_loader_simple")
ec = importlib.import_module("vognet-pytorch_amd.extended_config")
engine_mod = importlib.import_module("vognet-pytorch_amd.engine")
main_dist = importlib.import_module("vognet-pytorch_amd.main_dist")

NEW_EXPORTS = ("vog_obj_restore", "vog_ctx_obj_videos", "vog_ctx_set_stats", "vog_ctx_obj_band_rows")


def test_batch_and_restore_structs_match_the_c_header(tmp_path):
    """sizeof and the offset of EVERY member of vog_batch (which gained obj_out) and of the new vog_objrestore_args,
    as gcc lays them out, against the ctypes mirrors."""
    pairs = {"vog_batch": L.Batch, "vog_objrestore_args": L.ObjrestoreArgs}
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "vog_hip.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        src.append(f'  printf("{cname} - %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            src.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    src.append('  printf("VOG_ABI_VERSION - %d\\n", VOG_ABI_VERSION);')
    src += ['  return 0;', '}']
    (tmp_path / "abi.c").write_text("\n".join(src))
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")], check=True)
    out = subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    seen = set()
    for line in out:
        cname, fname, val = line.split()
        if cname == "VOG_ABI_VERSION":
            assert int(val) == 1                                   # an added optional field: the version stays
        elif fname == "-":
            assert C.sizeof(pairs[cname]) == int(val), (cname, C.sizeof(pairs[cname]), val)
        else:
            assert getattr(pairs[cname], fname).offset == int(val), (cname, fname, val)
            seen.add((cname, fname))
    assert ("vog_batch", "obj_out") in seen
    # the header puts it in front of `stats`: the three members the encoded inputs' layout test pins stay the last three
    assert [f for f, _ in L.Batch._fields_][-5:] == ["fault", "obj_out", "stats", "enc_prop", "enc_seg"]


def test_new_exports_are_built_and_declared():
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vog_hip.h")).read(), flags=re.S)
    for n in NEW_EXPORTS:
        assert hasattr(lib, n), f"libvog_hip.so does not export {n}"
        assert n in L.SYMBOLS and re.search(rf"\bint\s+{n}\s*\(", hdr), n
    assert lib.vog_version() == 1


def _ctx(**over):
    cfg = ec.get_default_cfg()
    ec.update_from_dict(cfg, over)
    desc = engine_mod.model_desc_from_cfg(cfg, {"vocab_size": 5000, "num_prop_per_frm": 5})
    h = C.c_void_p()
    lib = L.load()
    assert lib.vog_ctx_create(C.byref(desc), C.byref(h)) == 0
    return lib, h


def _err(lib):
    return (lib.vog_last_error() or b"").decode()


def test_forward_refuses_obj_out_by_rule_before_any_device_work():
    """The pointer checks of vog_batch come before anything needs a device: rc < 0 and a message that names the rule."""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    lib, h = _ctx(**{"mdl.name": "vog", "ds.conc_type": "sep"})
    try:
        b = L.Batch()
        b.B, b.ncmp, b.T = 1, 4, 3
        b.obj_out = p                                                  # without the segment encodings
        assert lib.vog_forward(h, C.byref(b), p, 256, None) < 0 and "obj_out comes with enc_seg" in _err(lib)
        b.enc_seg, b.enc_prop = p, p                                   # next to the encoded proposal rows
        assert lib.vog_forward(h, C.byref(b), p, 256, None) < 0 and "not next to them" in _err(lib)
        b.enc_prop, b.pad_region_feature = None, p                     # next to raw features (either of them)
        assert lib.vog_forward(h, C.byref(b), p, 256, None) < 0 and "not next to them" in _err(lib)
        b.pad_region_feature, b.seg_feature_for_frms = None, p
        assert lib.vog_forward(h, C.byref(b), p, 256, None) < 0 and "not next to them" in _err(lib)
        b.seg_feature_for_frms = None                                  # the pair alone passes these checks (and stops at the next
        assert lib.vog_forward(h, C.byref(b), p, 256, None) < 0        # one: the context has no weights yet)
        for rule in ("obj_out", "both or neither", "neither raw"):
            assert rule not in _err(lib) and _err(lib)
        buf2 = C.create_string_buffer(64)
        assert lib.vog_describe_steps(h, C.byref(L.Batch(B=1, ncmp=1, T=1, obj_out=p)), p, 256, 0, buf2, 64) < 0
        assert "obj_out comes with enc_seg" in _err(lib)
        # the older rules are what they were
        assert lib.vog_forward(h, C.byref(L.Batch(B=1, ncmp=1, T=1, enc_seg=p)), p, 256, None) < 0 and "both or neither" in _err(lib)
        assert lib.vog_forward(h, C.byref(L.Batch(B=1, ncmp=1, T=1)), p, 256, None) < 0 and "neither raw features" in _err(lib)
    finally:
        lib.vog_ctx_destroy(h)
    # contexts whose obj_tx is not per video, or that have none: the message says what already covers them
    for over in ({"mdl.name": "vog", "ds.conc_type": "spat"}, {"mdl.name": "vog", "ds.conc_type": "temp"},
                 {"mdl.name": "igrnd", "ds.conc_type": "sep"}, {"mdl.name": "vog", "ds.conc_type": "sep", "mdl.obj_tx.to_use": False}):
        lib, h = _ctx(**over)
        try:
            b = L.Batch(B=1, ncmp=4, T=3, obj_out=p, enc_seg=p)
            assert lib.vog_forward(h, C.byref(b), p, 256, None) < 0
            assert "sep / svsq model with an object transformer" in _err(lib) and "EncodedBank already covers" in _err(lib), over
            assert lib.vog_ctx_obj_videos(h, 1, 4, p, p, p, p, p, p, 256, None) < 0
            assert "sep / svsq model with an object transformer" in _err(lib), over
        finally:
            lib.vog_ctx_destroy(h)


def test_obj_videos_and_restore_argument_errors():
    lib, h = _ctx(**{"mdl.name": "vog", "ds.conc_type": "svsq"})
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    try:
        for B, ncmp in ((0, 4), (4, 0), (-1, 1)):
            assert lib.vog_ctx_obj_videos(h, B, ncmp, p, p, p, p, p, p, 256, None) < 0
            assert "geometry" in _err(lib), _err(lib)
        assert lib.vog_ctx_obj_videos(None, 1, 1, p, p, p, p, p, p, 256, None) < 0 and "bad argument" in _err(lib)
        for hole in range(6):                                          # every pointer is required
            a = [p] * 6
            a[hole] = None
            assert lib.vog_ctx_obj_videos(h, 1, 1, a[0], a[1], a[2], a[3], a[4], a[5], 256, None) < 0 and "bad argument" in _err(lib)
        assert lib.vog_ctx_obj_videos(h, 1, 1, p, p, p, p, p, p, 256, None) < 0 and "finalized" in _err(lib)
        assert lib.vog_ctx_set_stats(None, p) < 0 and lib.vog_ctx_set_stats(h, None) == 0
        assert lib.vog_ctx_obj_band_rows(None) < 0 and lib.vog_ctx_obj_band_rows(h) < 0          # (not finalized)
    finally:
        lib.vog_ctx_destroy(h)
    assert lib.vog_obj_restore(None, None) < 0 and "bad argument" in _err(lib)
    a = L.ObjrestoreArgs()
    assert lib.vog_obj_restore(C.byref(a), None) < 0
    a.x = a.y16 = p
    a.n_rows, a.nppf0, a.d_obj, a.seg_enc, a.ldc = 10, 3, 16, 8, 16    # rows not a multiple of nppf0
    assert lib.vog_obj_restore(C.byref(a), None) < 0 and "bad argument" in _err(lib)
    a.n_rows, a.ldc = 9, 12                                            # a row pitch narrower than the row
    assert lib.vog_obj_restore(C.byref(a), None) < 0 and "bad argument" in _err(lib)
    a.ldc, a.y16, a.y16_lo = 16, None, p                               # a remainder without the rows it is the remainder of
    assert lib.vog_obj_restore(C.byref(a), None) < 0 and "bad argument" in _err(lib)
    a.y16, a.prop_seg = p, p                                           # the segment part without its source
    assert lib.vog_obj_restore(C.byref(a), None) < 0 and "bad argument" in _err(lib)
    a.prop_seg, a.enc_seg, a.seg_enc = p, p, 16                        # no proposal columns left
    assert lib.vog_obj_restore(C.byref(a), None) < 0 and "bad argument" in _err(lib)


def test_engine_side_key_checks_need_no_device():
    fk = engine_mod.feature_kind
    OBJ, ENC = engine_mod.OBJ_KEYS, engine_mod.ENC_KEYS
    assert OBJ == ("obj_region_feature", "enc_seg_feature")
    assert fk({"pad_region_feature": 0, "seg_feature_for_frms": 0}) == "raw"
    assert fk({ENC[0]: 0, ENC[1]: 0, "pad_proposals": 0}) == "enc"
    assert fk({OBJ[0]: 0, OBJ[1]: 0, "pad_proposals": 0}) == "obj"
    with pytest.raises(ValueError, match="pair"):                      # half a pair, either half
        fk({OBJ[0]: 0})
    with pytest.raises(ValueError, match="pair"):
        fk({OBJ[1]: 0})
    for extra in ("pad_region_feature", "seg_feature_for_frms", ENC[0]):
        with pytest.raises(ValueError, match="never a mix"):
            fk({OBJ[0]: 0, OBJ[1]: 0, extra: 0})
    with pytest.raises(ValueError, match="not both"):                  # the older rule, in its own words
        fk({ENC[0]: 0, ENC[1]: 0, "pad_region_feature": 0})
    assert engine_mod.has_encodings({ENC[0]: 0, ENC[1]: 0}) is True
    assert (dls.ObjBank.region_key, dls.ObjBank.seg_key) == OBJ
    assert issubclass(dls.ObjBank, dls.EncodedBank) and dls.EncodedBank.region_key == ENC[0]


def test_bytes_per_video_of_obj_rows():
    """gt5: 50 rows of 512 and 10 segment rows of 256 fp32 values = 102,400 + 10,240 = 112,640 B (encoded bank: 61,440 B);
    100 proposals per frame: 2,048,000 + 10,240 = 2,058,240 B; the small tables are the parent's."""
    OB, EB, FB = dls.ObjBank, dls.EncodedBank, dls.FeatureBank
    small = {n: 10 * n * (7 * 4 + 1) + 100 * 5 * 4 + 8 for n in (5, 100)}
    assert OB.bytes_per_video(5, 256, 256, 100) - small[5] == 112_640
    assert EB.bytes_per_video(5, 256, 256, 100) - small[5] == 61_440
    assert OB.bytes_per_video(100, 256, 256, 100) - small[100] == 2_058_240
    for nppf0 in (5, 100):
        assert OB.bytes_per_video(nppf0, 256, 256, 100) == FB.bytes_per_video(nppf0, 512, 256, 100, "f32")
    assert OB.bytes_per_video(5, 32, 16, 8, nfrm0=4) == 4 * (5 * 48 + 16) * 4 + 4 * 5 * 29 + 8 * 20 + 8
    with pytest.raises(ValueError, match="fp32"):
        OB.bytes_per_video(5, 256, 256, 100, "f16")


def test_obj_bank_refuses_other_models_at_construction():
    """Before any table is allocated: the configuration alone says whether obj_tx sees one video at a time."""
    for over in ({"mdl.name": "vog", "ds.conc_type": "spat"}, {"mdl.name": "vog", "ds.conc_type": "temp"},
                 {"mdl.name": "igrnd", "ds.conc_type": "sep"}, {"mdl.name": "vog", "ds.conc_type": "svsq", "mdl.obj_tx.to_use": False}):
        cfg = ec.get_default_cfg()
        ec.update_from_dict(cfg, over)
        with pytest.raises(ValueError, match="EncodedBank already covers"):
            dls.ObjBank(cfg, {"num_prop_per_frm": 5}, 4)


def test_cli_keyword_parses_and_refuses():
    uid, kw = main_dist.parse_argv(["exp1", "--feature_bank=obj", "--feature_bank_videos=32", "--only_val"])
    assert uid == "exp1" and kw["feature_bank"] == "obj" and kw["feature_bank_videos"] == "32" and kw["only_val"] == "True"
    assert "--feature_bank=obj" in main_dist.__doc__
    # the refusals come before the model is built: SystemExit with the rule as its text
    for over in ({"ds.conc_type": "spat"}, {"ds.conc_type": "temp"}, {"ds.conc_type": "sep", "mdl.name": "igrnd"}):
        with pytest.raises(SystemExit, match="EncodedBank already covers"):
            main_dist.main_dist("exp1", feature_bank="obj", only_val="True", **over)
    with pytest.raises(SystemExit, match="needs --feature_bank"):
        main_dist.main_dist("exp1", query_bank="True", only_val="True")
