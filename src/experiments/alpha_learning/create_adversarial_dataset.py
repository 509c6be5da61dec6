from gen_adversarial_amd.experiments.alpha_learning.create_adversarial_dataset import (L2_BOUNDS, build_defender, create, main,  # noqa: F401
                                                                                       named_folder_dataset, parse_args, save_adversary)

if __name__ == '__main__':
    main(parse_args())
