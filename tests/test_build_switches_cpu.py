"""Build switches named in the documents and tools exist in the kernel sources, and the retired ablation switches stay retired
(plain text scan, no compiler).  HISTORY.md and profiles/ record the past and are left out."""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "multiply_amd", "csrc")
TEXT = (".py", ".hip", ".hpp", ".h", ".sh", ".md", ".txt")

# the experiment switches that remain: instrumentation with tools of its own, and variants whose question is open
KEPT_EXP = {"MP_EXP_STAMP", "MP_EXP_SIG16", "MP_EXP_SIGBITS"}
# retired switches outside the MP_EXP_* / TF_EXP families
RETIRED = {"MP_DMA_ONE_M0", "MP_DMA_SPLIT", "MP_DMA_LATE", "MP_DMA_EARLY", "MP_NT_PERSIST", "MP_NT_WIDE", "MP_NT_SWZ"}


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _csrc_text():
    return "\n".join(_read(p) for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))))


def _tree(*roots):
    for root in roots:
        root = os.path.join(REPO, root)
        if os.path.isfile(root):
            yield root
            continue
        for d, dirs, files in os.walk(root):
            dirs[:] = [x for x in dirs if not x.startswith("_build") and x not in ("__pycache__", "ab_libs", "bin")]
            for f in files:
                if f.endswith(TEXT):
                    yield os.path.join(d, f)


def test_documented_switches_exist():
    """every -D<NAME> in tools/README.md, tools/*.py, tools/*.sh, DESIGN.md and README.md is a name the kernel sources know"""
    files = [os.path.join(REPO, f) for f in ("tools/README.md", "DESIGN.md", "README.md")]
    files += sorted(glob.glob(os.path.join(REPO, "tools", "*.py")) + glob.glob(os.path.join(REPO, "tools", "*.sh")))
    names = set(re.findall(r"\b[A-Za-z_]\w*", _csrc_text()))
    missing = {}
    for path in files:
        for name in re.findall(r"(?<![\w-])-D([A-Z][A-Z0-9_]*)", _read(path)):
            if name not in names:
                missing.setdefault(os.path.relpath(path, REPO), set()).add(name)
    assert not missing, f"-D switches that multiply_amd/csrc/ does not know: {missing}"


def test_retired_switches_stay_retired():
    """no MP_EXP_* / TF_EXP token outside the kept list, and no other retired switch, in the sources, tools and documents"""
    assert KEPT_EXP <= set(re.findall(r"\bMP_EXP_\w+", _csrc_text())), "a kept switch left the kernel sources: update KEPT_EXP"
    found = {}
    for path in _tree("multiply_amd", "tools", "include", "README.md", "DESIGN.md", "INTEGRATION.md"):
        for name in re.findall(r"\b(?:MP_EXP_\w+|TF_EXP\w*|MP_DMA_\w+|MP_NT_\w+)", _read(path)):
            if (name.startswith(("MP_EXP_", "TF_EXP")) and name not in KEPT_EXP) or name in RETIRED:
                found.setdefault(os.path.relpath(path, REPO), set()).add(name)
    assert not found, f"retired build switches are back: {found}"
