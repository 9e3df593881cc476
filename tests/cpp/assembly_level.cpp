// BilinearForm::SetAssemblyLevel in the reference's call forms: every level is accepted, LEGACY and FULL mark
// the form as assembled (the CSR operator on quads / hexes), the others keep partial assembly.  Compiled and
// linked with the drivers' flags (tests/test_cpp_fa_tensor.py); nothing here touches a device.
#include "mfem.hpp"

using namespace mfem;

int main(int argc, char *argv[])
{
    Mpi::Init(argc, argv);
    Mesh mesh = Mesh::MakeCartesian2D(2, 2, Element::QUADRILATERAL);
    ParMesh pmesh(MPI_COMM_WORLD, mesh);
    H1_FECollection fec(2, 2);
    ParFiniteElementSpace fespace(&pmesh, &fec);
    ParBilinearForm a(&fespace);
    int bad = a.Assembled() ? 1 : 0;  // no call: partial assembly
    a.SetAssemblyLevel(AssemblyLevel::LEGACY);
    bad += a.Assembled() ? 0 : 1;
    a.SetAssemblyLevel(AssemblyLevel::PARTIAL);
    bad += a.Assembled() ? 1 : 0;
    a.SetAssemblyLevel(AssemblyLevel::FULL);
    bad += a.Assembled() ? 0 : 1;
    a.SetAssemblyLevel(AssemblyLevel::ELEMENT);
    a.SetAssemblyLevel(AssemblyLevel::NONE);
    bad += a.Assembled() ? 1 : 0;
    return bad;
}
