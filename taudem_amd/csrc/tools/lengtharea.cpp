// lengtharea -plen plen -ad8 ad8 -ss ss [-par M y] | lengtharea base   (argument surface of src/LengthAreamn.cpp:50-133; -par defaults 0.03 1.3)
#include "indices_args.hpp"

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    cli::IndexArgs a;
    if (!cli::parse_index_args(cli::kLengthArea, argc, argv, a)) return cli::index_usage(cli::kLengthArea, argv[0]);
    const int err = tdx_tool_lengtharea(a.file[0].c_str(), a.file[1].c_str(), a.file[2].c_str(), a.par);
    if (err != 0 && !cli::is_abort_code(err)) { printf("Length Area Error %d\n", err); return 0; }
    return cli::finish("Length Area", err);
}
