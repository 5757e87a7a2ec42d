// editraster -in raster -out newraster -changes changefile   (argument surface of src/EditRastermn.cpp:50-100; no simple use)
#include "cli_common.hpp"

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string rasterfile, newfile, changefile;
    bool ok = argc > 2;
    int i = 1;
    while (ok && argc > i) {
        std::string* dst = strcmp(argv[i], "-in") == 0 ? &rasterfile : strcmp(argv[i], "-out") == 0 ? &newfile : strcmp(argv[i], "-changes") == 0 ? &changefile : nullptr;
        i++;
        if (!dst || argc <= i) ok = false;
        else *dst = argv[i++];
    }
    if (!ok) {
        printf("Editraster use:\n %s -in <filetochange>\n", argv[0]);
        printf("-out <filetowrite> \n");
        printf("-changes <file with change values (x,y,newvalue)> \n");
        return 0;
    }
    const int err = tdx_tool_editraster(rasterfile.c_str(), newfile.c_str(), changefile.c_str());
    // the reference's main says "Threshold Error" here (src/EditRastermn.cpp:91-92)
    if (err != 0 && !cli::is_abort_code(err)) { printf("Threshold Error %d\n", err); return 0; }
    return cli::finish("Editraster", err);
}
