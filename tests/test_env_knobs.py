"""The KP_* environment variables of the native sources stay in one place: getenv is called
only by the two helpers of karmada_amd/csrc/kp_env.h, and the table at the top of that header
lists exactly the variables the sources pass to them."""
import os
import re

from karmada_amd.engine import PKG

CSRC = os.path.join(PKG, "csrc")
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".cpp", ".hip")))


def read(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def test_getenv_only_in_kp_env():
    assert "kp_env.h" in SOURCES
    users = [f for f in SOURCES if "getenv(" in read(f)]
    assert users == ["kp_env.h"], users


def test_knob_table_matches_the_reads():
    used = set()
    for f in SOURCES:
        used |= set(re.findall(r'\bkp_env_(?:int|flag)\(\s*"(KP_[A-Z0-9_]+)"', read(f)))
    # every helper call names its variable with a literal (none is hidden from the scan above)
    for f in SOURCES:
        if f != "kp_env.h":
            assert not re.search(r'\bkp_env_(?:int|flag)\(\s*[^"\s]', read(f)), f
    table = set(re.findall(r"^//   (KP_[A-Z0-9_]+) ", read("kp_env.h"), flags=re.M))
    assert used and used == table, (sorted(used - table), sorted(table - used))
