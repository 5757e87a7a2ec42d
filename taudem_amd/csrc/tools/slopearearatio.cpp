// slopearearatio -slp slp -sca sca -sar sar | slopearearatio base   (argument surface of src/SlopeAreaRatiomn.cpp:48-129)
#include "indices_args.hpp"

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    cli::IndexArgs a;
    if (argc < 2) printf("Error: To run this program, use either the Simple Usage option or\nthe Usage with Specific file names option\n");
    if (!cli::parse_index_args(cli::kSlopeAreaRatio, argc, argv, a)) return cli::index_usage(cli::kSlopeAreaRatio, argv[0]);
    const int err = tdx_tool_slopearearatio(a.file[0].c_str(), a.file[1].c_str(), a.file[2].c_str());
    if (err != 0 && !cli::is_abort_code(err)) { printf("Slope area ratio error %d\n", err); return 0; }
    return cli::finish("Slope area ratio", err);
}
