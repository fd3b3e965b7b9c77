"""``tests/spgto_harness.py`` bound to the route of csrc/spdgto.hip -- a helper, no test: ``Basis`` with the shells and the
normalisation of ``gto_spd`` (l <= 2), whose ``run`` / ``run_dipole`` call ``evc_spdgto_integrals_batch`` /
``evc_spdgto_dipole_batch``.  The molecules are in tests/spdgto_cases.py."""
import spgto_harness
from spgto_harness import (DEV, ENERGY, ENERGY_FIELDS, FENCE, GRAD_FIELDS, GUARD, S2KL, S4, Fenced, pack_eri,  # noqa: F401
                           pack_ip1, run, run_dipole, shapes)


class Basis(spgto_harness.Basis):
    route = "spdgto"
