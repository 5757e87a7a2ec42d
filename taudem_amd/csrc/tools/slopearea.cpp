// slopearea -slp slp -sca sca -sa sa [-par m n] | slopearea base   (argument surface of src/SlopeAreamn.cpp:50-133; -par defaults 2 1)
#include "indices_args.hpp"

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    cli::IndexArgs a;
    if (!cli::parse_index_args(cli::kSlopeArea, argc, argv, a)) return cli::index_usage(cli::kSlopeArea, argv[0]);
    const int err = tdx_tool_slopearea(a.file[0].c_str(), a.file[1].c_str(), a.file[2].c_str(), a.par);
    if (err != 0 && !cli::is_abort_code(err)) { printf("SlopeArea Error %d\n", err); return 0; }
    return cli::finish("SlopeArea", err);
}
