// setregion -p p -gw gw -out out [-id n]   (argument surface of src/SetRegionmn.cpp:50-113; -id defaults to 1, no simple use)
#include "indices_args.hpp"

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    cli::IndexArgs a;
    if (!cli::parse_index_args(cli::kSetRegion, argc, argv, a)) return cli::index_usage(cli::kSetRegion, argv[0]);
    const int err = tdx_tool_setregion(a.file[0].c_str(), a.file[1].c_str(), a.file[2].c_str(), a.id);
    // the reference prints the truth value of (err != 0), not the code
    if (err != 0 && !cli::is_abort_code(err)) { printf("Set Region Error %d\n", 1); return 0; }
    return cli::finish("Set Region", err);
}
