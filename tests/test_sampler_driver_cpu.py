"""The sampler's host driver lives in multiply_amd/ray_sampler.py (SamplerRun, sample_persons): its state is named up front, no
mode flag tells it whose weights to use, and Multiply keeps only the delegates."""
import ast
import glob
import os

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multiply_amd")


def _class(module, name):
    with open(os.path.join(PKG, module)) as f:
        tree = ast.parse(f.read())
    found = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name]
    assert len(found) == 1, (module, name)
    return found[0]


def _methods(cls):
    return {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}


def _self_attributes_stored(fn):
    return {n.attr for n in ast.walk(fn) if isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Store)
            and isinstance(n.value, ast.Name) and n.value.id == "self"}


def test_sampler_run_names_all_its_fields_up_front():
    from multiply_amd.ray_sampler import SamplerRun
    cls = _class("ray_sampler.py", "SamplerRun")
    methods = _methods(cls)
    assert {"__init__", "query", "sdf", "resample", "close"} <= set(methods)
    slots = set(SamplerRun.__slots__)
    assert len(slots) == len(SamplerRun.__slots__) and "__dict__" not in slots
    assert SamplerRun.__bases__ == (object,) and "__dict__" not in vars(SamplerRun)      # instances have no attribute dict at all
    in_init = _self_attributes_stored(methods["__init__"])
    assert in_init == slots, (sorted(slots - in_init), sorted(in_init - slots))       # every field is set by the constructor
    for name, fn in methods.items():
        if name != "__init__":
            assert _self_attributes_stored(fn) <= in_init, (name, sorted(_self_attributes_stored(fn) - in_init))
    for fn in methods.values():                                                          # ... and nothing goes through setattr
        assert not [n for n in ast.walk(fn) if isinstance(n, ast.Call) and ast.unparse(n.func) in ("setattr", "object.__setattr__")]


def test_no_training_mode_flag_is_left_in_the_package():
    for path in sorted(glob.glob(os.path.join(PKG, "**", "*"), recursive=True)):
        if os.path.isfile(path) and "__pycache__" not in path:
            with open(path, "rb") as f:
                assert b"_mp_in_train_graph" not in f.read(), path


def test_multiply_keeps_the_delegates_and_none_of_the_driver():
    methods = _methods(_class("multiply.py", "Multiply"))
    removed = {"_sampler_cfg", "_sampler_open", "_sampler_query", "_sampler_sdf", "_sampler_resample", "_sampler_close",
               "_vote_groups_check"}
    assert not removed & set(methods)
    assert {"_sample_persons", "_sample_person", "sample_rays", "resolved_sampler_sdf_mode", "_setup"} <= set(methods)

    def params(name):
        a = methods[name].args
        return [x.arg for x in a.args], len(a.defaults)
    assert params("_sample_persons") == (["self", "cx", "draws_by_person", "persons", "shared_lins"], 3)
    assert params("_sample_person") == (["self", "cx", "n", "p", "draws"], 1)
    assert params("resolved_sampler_sdf_mode") == (["self", "p"], 1)
    assert params("_setup") == (["self", "input", "id", "canonical_pose", "side_stream", "host_hull"], 2)
    init = ast.unparse(methods["__init__"])
    for attr in ("sampler_sdf_mode", "sampler_vote_group", "convergence_group"):
        assert f"self.{attr} = " in init, attr
    for name in ("_sample_persons", "_sample_person"):                                  # delegates of a few lines
        assert methods[name].end_lineno - methods[name].lineno < 8, name
